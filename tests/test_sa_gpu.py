"""The smoothed-aggregation setup on an MI355X (-m gpu): learnmultigrid_amd/aggregation.py and csrc/sa.hip against the
plain-Python twin of their rules (tests/sa_ref.py) -- every integer equal, every value bit for bit --, on the case matrices
and edge shapes of tests/sa_cases.py; then whole hierarchies through solvers.SmoothedAggregationAMG against the oracle's
cycle on the twin's transfers, and the hierarchy as a preconditioner of CG and GMRES.

Each whole-hierarchy test prints its largest relative deviation from the oracle's history before it asserts."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import block_cg_ref                                                # noqa: E402
import sa_cases as C                                               # noqa: E402
import sa_ref as R                                                 # noqa: E402
from learnmultigrid_amd import aggregation as agn, amg, ops        # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy                 # noqa: E402
from learnmultigrid_amd.solvers import CG, GMRES, SmoothedAggregationAMG   # noqa: E402
from support import DEV, dev                                       # noqa: E402

CASES = sorted(C.case_matrices())
RTOL, FLOOR = 1e-10, 1e-14                                          # the bound of tests/test_amg_gpu.py (deviation below)


def tensors(M):
    return M.rowptr, M.colidx, M.vals


def assert_csr_equal(got, want, what):
    """The DeviceCSR `got` is the SciPy CSR `want`: shape, integers, and the values bit for bit."""
    rp, ci, va = (t.cpu().numpy() for t in tensors(got))
    assert got.shape == want.shape, what
    assert np.array_equal(rp, want.indptr) and np.array_equal(ci, want.indices), what
    assert np.array_equal(va.view(np.int64), want.data.view(np.int64)), what


def assert_same(a, b, what):
    assert a.shape == b.shape and all(torch.equal(x, y) for x, y in zip(tensors(a), tensors(b))), what


def bits(t):
    return t.cpu().numpy().view(np.int64)


# ---- stage parity against the twin, edge shapes included -----------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_stages_are_the_twins_integers_and_bits(name):
    A, theta, _ = C.case_matrices()[name]
    B = C.candidate(name)
    n = A.shape[0]
    dA, dB = ops.DeviceCSR.from_scipy(A, DEV), dev(B)
    # strength and the aggregation graph
    S = R.symmetric_strength(A, theta)
    dS = agn.symmetric_strength_device(dA, theta)
    assert_csr_equal(dS, S, "S")
    assert_same(agn.symmetric_strength_device(dA, theta), dS, "S twice")
    agg, n_agg, rounds, state, G = R.aggregate(S)
    dG = agn.graph_device(dS)
    assert_csr_equal(dG, G, "G")
    assert_same(agn.graph_device(dS), dG, "G twice")
    # roots and aggregates
    parts = {}
    d_agg, d_n_agg, d_rounds = agn.aggregate_device(dS, parts)
    assert (d_n_agg, d_rounds) == (n_agg, rounds)
    assert np.array_equal(parts["state"].cpu().numpy(), state) and np.array_equal(d_agg.cpu().numpy(), agg)
    assert_csr_equal(parts["G"], G, "G of aggregate_device")
    again = agn.aggregate_device(dS)
    assert torch.equal(again[0], d_agg) and again[1:] == (d_n_agg, d_rounds)
    if n_agg in (0, n):
        assert agn.transfer_device(dA, dB, theta)[:2] == (None, None)
        return
    # the tentative prolongator and the coarse candidate
    T, Bc = R.tentative(agg, n_agg, B)
    dT, dBc = agn.tentative_device(d_agg, d_n_agg, dB)
    assert_csr_equal(dT, T, "T")
    assert np.array_equal(bits(dBc), Bc.view(np.int64)), "Bc"
    dT2, dBc2 = agn.tentative_device(d_agg, d_n_agg, dB)
    assert_same(dT2, dT, "T twice")
    assert torch.equal(dBc2, dBc)
    # the Jacobi step on T: the default damping, another one, and none (plain aggregation)
    for omega in (4.0 / 3.0, 0.7, 0.0):
        P = R.smooth_prolongator(A, T, agg, omega)
        dP = agn.smooth_prolongator_device(dA, dT, omega)
        assert_csr_equal(dP, P, "P at omega %r" % omega)
        assert_same(agn.smooth_prolongator_device(dA, dT, omega), dP, "P twice")
    assert agn.jacobi_scale(dA) == R.jacobi_scale(A)
    # the level as a whole
    P, Bc, info, _ = R.transfer(A, B, theta)
    dP, dBc, d_info = agn.transfer_device(dA, dB, theta)
    assert_csr_equal(dP, P, "P of transfer_device")
    assert np.array_equal(bits(dBc), Bc.view(np.int64)) and d_info == info


def test_a_candidate_that_vanishes_on_an_aggregate_is_refused_with_its_row():
    A, B, row = C.zero_candidate()
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    with pytest.raises(amg.Refused) as e:
        agn.transfer_device(dA, dev(B))
    assert (e.value.rule, e.value.row) == ("candidate", row)
    with pytest.raises(R.Refused) as e:
        R.transfer(A, B)
    assert (e.value.rule, e.value.row) == ("candidate", row)
    with pytest.raises(amg.Refused):
        agn.sa_hierarchy(A, DEV, B=B, max_coarse=2)
    # a candidate that is not finite on one aggregate and zero on another: the smallest row of the two
    bad = B.copy()
    bad[0] = np.inf
    with pytest.raises(amg.Refused) as e:
        agn.transfer_device(dA, dev(bad))
    assert (e.value.rule, e.value.row) == ("candidate", 0)


def test_keywords_are_checked_on_the_host():
    dA = ops.DeviceCSR.from_scipy(C.chain(5), DEV)
    for kw in (dict(theta=-0.1), dict(theta=1.5), dict(omega=float("nan")), dict(max_levels=0), dict(B=np.ones(4))):
        with pytest.raises(ValueError):
            agn.sa_hierarchy(dA, DEV, max_coarse=2, **kw)
    with pytest.raises(TypeError):
        agn.sa_hierarchy(dA, DEV, split="pmis")
    with pytest.raises(TypeError):
        SmoothedAggregationAMG(C.chain(5), np.ones((5, 1)), interp_trunc=0.2)
    H = agn.sa_hierarchy(dA, DEV, max_coarse=2, B=np.arange(1.0, 6.0))
    assert H.sizes == [5, 1] and H.amg_info[0]["n_agg"] == 1 and H.amg_info[1] == {"n": 1, "nnz": 1, "n_agg": None, "rounds": None}


# ---- whole hierarchies --------------------------------------------------------------------------------------------------------
SOLVE = dict(smoother="Jacobi", smooth_steps=2, omega=0.8, smoother_semantics="as_named")


def deviation(got, want, largest):
    """The largest |got - want| in units of the bound of tests/test_amg_gpu.py: 1e-10 relative with a floor of 1e-14 of
    `largest` = ||b||, the residual the run starts from."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / (RTOL * np.abs(want) + FLOOR * largest)))


def solver_for(name, **kw):
    A, b = C.problems()[name]
    return SmoothedAggregationAMG(A, b.reshape(-1, 1).copy(), **dict(C.SA_KW, theta=C.THETA[name], **kw)), A, b


@functools.lru_cache(maxsize=None)
def jacobi_history(name):
    A, b = C.problems()[name]
    return C.oracle_history(A, b, C.twin_hierarchy(name)[0], cap=C.CAP)


@pytest.mark.parametrize("name", sorted(C.problems()))
def test_sa_solve_matches_the_oracle_on_the_twins_transfers(name):
    """V(2,2) damped Jacobi (0.8), max_coarse=100, to 1e-8 ||b|| (the anisotropic problem at theta 0.25): the level sizes of
    the twin, the oracle's residual history within 1e-10 relative, the twin's cycle count (tests/test_sa_cpu.py: 31 .. 50)."""
    mg, A, b = solver_for(name)
    Ps, As, infos = C.twin_hierarchy(name)
    want = jacobi_history(name)
    mg.solve(max_iterations=C.CAP + 1, error=C.TARGET * np.linalg.norm(b), **SOLVE)
    assert mg.level_dims == [M.shape[0] for M in As]
    got = mg.get_track_res().ravel()
    assert got[0] == np.sqrt(A.shape[0])                           # (the reference's first entry)
    print("%s: levels %s, %d cycles, deviation %.3f of the bound" % (name, mg.level_dims, got.size - 1, deviation(got[1:], want[1:], want[0])))
    assert deviation(got[1:], want[1:], want[0]) <= 1.0
    assert got.size - 1 == C.cycles_needed(want) <= C.CAP and got[-1] <= C.TARGET * np.linalg.norm(b)
    info = mg.hierarchy_info()
    assert [(d["n"], d["nnz"]) for d in info["levels"]] == [(M.shape[0], M.nnz) for M in As]
    assert [(d["n_agg"], d["rounds"]) for d in info["levels"][:len(infos)]] == [(d["n_agg"], d["rounds"]) for d in infos]
    assert all(d["n_agg"] is None and d["rounds"] is None for d in info["levels"][len(infos):])
    assert info["operator_complexity"] == sum(M.nnz for M in As) / As[0].nnz
    assert info["grid_complexity"] == sum(M.shape[0] for M in As) / As[0].shape[0]
    # the transfers stayed on the device and are the twin's, bit for bit
    for lev, Pt in zip(mg._hier.levels, Ps):
        assert_csr_equal(lev.P, Pt, "P")


def test_gauss_seidel_as_shipped():
    mg, A, b = solver_for("jittered")
    want = C.oracle_history(A, b, C.twin_hierarchy("jittered")[0], cap=C.CAP, smoother="GaussSeidel", steps=2)
    mg.solve(smooth_steps=2, max_iterations=C.CAP + 1, error=C.TARGET * np.linalg.norm(b))
    got = mg.get_track_res().ravel()
    print("Gauss-Seidel: %d cycles, deviation %.3f of the bound" % (got.size - 1, deviation(got[1:], want[1:], want[0])))
    assert deviation(got[1:], want[1:], want[0]) <= 1.0
    assert got.size - 1 == C.cycles_needed(want) <= C.CAP


def test_solve_many_and_gmres_on_one_hierarchy():
    mg, A, b = solver_for("jittered")
    nb = np.linalg.norm(b)
    want = jacobi_history("jittered")
    v_cycles = C.cycles_needed(want)
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
    g.solve(max_iterations=C.CAP, error=C.TARGET * nb, restart=10, preconditioner=H, precond_steps=2, precond_omega=0.8)
    print("GMRES(10): %d iterations against %d cycles" % (g.get_iterations(), v_cycles))
    assert g.get_residual() <= C.TARGET * nb and g.get_iterations() < v_cycles
    assert np.linalg.norm(b.ravel() - A @ g.get_solution().ravel()) <= 2 * C.TARGET * nb
    Bs = b.reshape(-1, 1) * scale[:3]
    X, _ = GMRES(A, b.reshape(-1, 1).copy()).solve_many(Bs, max_iterations=C.CAP, error=C.TARGET * nb * 0.5, restart=10, preconditioner=H,
                                                        precond_steps=2, precond_omega=0.8)
    for j in range(3):
        assert np.linalg.norm(Bs[:, j] - A @ X[:, j]) <= 2 * C.TARGET * nb * abs(scale[j])


def test_cg_converges_with_the_hierarchy_as_preconditioner():
    """The symmetric problem of the block-CG tests (block_cg_ref.problem: the jittered operator with the Dirichlet couplings
    eliminated, so its boundary rows are isolated nodes with empty rows of P), V(2,2) damped Jacobi as the preconditioner:
    CG reaches 1e-8 ||b|| within the 60 iterations the stationary cycles are given, and in fewer than plain CG."""
    A, _, B = block_cg_ref.problem()
    b = B[:, :1].copy()
    nb = np.linalg.norm(b)
    H = agn.sa_hierarchy(A, DEV, **C.SA_KW)
    assert len(H.sizes) >= 2 and H.amg_info[0]["n_agg"] == H.sizes[1]
    kw = dict(preconditioner=H, precond_steps=2, precond_omega=0.8)
    plain = CG(A, b.copy())
    plain.solve(max_iterations=2000, error=C.TARGET * nb)
    pcg = CG(A, b.copy())
    pcg.solve(max_iterations=C.CAP, error=C.TARGET * nb, **kw)
    print("CG: %d iterations preconditioned, %d plain" % (pcg.get_iterations(), plain.get_iterations()))
    assert pcg.get_residual() <= C.TARGET * nb and pcg.get_iterations() < min(C.CAP, plain.get_iterations())
    assert np.linalg.norm(b.ravel() - A @ pcg.get_solution().ravel()) <= 2 * C.TARGET * nb
    X, _ = CG(A, b.copy()).solve_many(B[:, :3], max_iterations=C.CAP, error=C.TARGET * nb, **kw)
    for j in range(3):
        assert np.linalg.norm(B[:, j] - A @ X[:, j]) <= 2 * C.TARGET * nb


def test_a_matrix_without_a_coarse_level_is_refused_by_the_solver():
    A = C.case_matrices()["diagonal"][0]
    H = agn.sa_hierarchy(A, DEV, max_coarse=2)
    assert H.sizes == [5] and H.amg_info[0]["n_agg"] == 0 and H.amg_info[0]["rounds"] == 0
    with pytest.raises(ValueError, match="no coarse level"):
        SmoothedAggregationAMG(A, np.ones((5, 1)), max_coarse=2).solve()
