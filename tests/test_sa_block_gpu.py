"""Smoothed aggregation for systems on an MI355X (-m gpu): learnmultigrid_amd/aggregation.py and csrc/nsp.hip against the
plain-Python twin of their rules (tests/nsp_ref.py) -- every integer equal, every value bit for bit -- on the cases of
tests/nsp_cases.py; the refusals with the row the twin names; then a whole hierarchy on elasticity_2d(16) through
solvers.SmoothedAggregationAMG against the oracle's cycle on the twin's transfers, and as a preconditioner of CG and GMRES.

The whole-hierarchy test prints its largest relative deviation from the oracle's history before it asserts."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import nsp_cases as NC                                             # noqa: E402
import nsp_ref as R                                                # noqa: E402
import sa_cases as SC                                              # noqa: E402
import sa_ref                                                      # noqa: E402
from learnmultigrid_amd import aggregation as agn, amg, ops        # noqa: E402
from learnmultigrid_amd.solvers import CG, GMRES, SmoothedAggregationAMG   # noqa: E402
from support import DEV, dev                                       # noqa: E402

CASES = sorted(NC.cases())
RTOL, FLOOR = 1e-10, 1e-14                                          # the bound of tests/test_amg_gpu.py


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


# ---- stage parity against the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_stages_are_the_twins_integers_and_bits(name):
    A, bs, X = NC.cases()[name]
    n, k = X.shape
    dA, dX = ops.DeviceCSR.from_scipy(A, DEV), dev(X)
    Pm, Bc, info, parts = R.transfer(A, X, bs=bs)
    # the condensed matrix, then the stages of sa.hip on it
    dC = agn.condense_device(dA, bs)
    assert_csr_equal(dC, parts["C"], "C")
    assert_same(agn.condense_device(dA, bs), dC, "C twice")
    dS = agn.symmetric_strength_device(dC, 0.0)
    assert_csr_equal(dS, parts["S"], "S")
    d_agg, d_n_agg, d_rounds = agn.aggregate_device(dS)
    assert (d_n_agg, d_rounds) == (info["n_agg"], info["rounds"]) and np.array_equal(d_agg.cpu().numpy(), parts["agg"])
    # the tentative prolongator of k candidates and the coarse candidates
    dT, dBc = agn.tentative_block_device(d_agg, d_n_agg, bs, dX)
    assert_csr_equal(dT, parts["T"], "T")
    assert dBc.shape == Bc.shape and np.array_equal(bits(dBc), Bc.view(np.int64)), "Bc"
    dT2, dBc2 = agn.tentative_block_device(d_agg, d_n_agg, bs, dX)
    assert_same(dT2, dT, "T twice")
    assert torch.equal(dBc2, dBc)
    # the level as a whole: the Jacobi step on T at the default damping and at none
    for omega in (4.0 / 3.0, 0.0):
        want = R.transfer(A, X, omega=omega, bs=bs)[0] if omega else sa_ref.smooth_prolongator(A, parts["T"], parts["rows"], 0.0)
        dP, dBc3, d_info = agn.transfer_device(dA, dX, 0.0, omega, bs)
        assert_csr_equal(dP, want, "P at omega %r" % omega)
        assert torch.equal(dBc3, dBc) and d_info == info
    assert_same(agn.transfer_device(dA, dX, block_size=bs)[0], agn.transfer_device(dA, dX, block_size=bs)[0], "P twice")


def test_condensation_counts_an_explicit_zero():
    A = R.canonical(NC.explicit_zero_block())
    dC = agn.condense_device(ops.DeviceCSR.from_scipy(A, DEV), 2)
    C = R.condense(A, 2)
    assert_csr_equal(dC, C, "C")
    assert C.nnz == 6 and C[0, 2] == 0.0 and dC.vals.cpu().numpy()[1] == 0.0
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    assert agn.condense_device(dA, 1) is dA
    with pytest.raises(ValueError):
        agn.condense_device(dA, 4)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NC.refusals()))
def test_deficient_candidates_are_refused_with_the_twins_row(name):
    A, bs, X, row = NC.refusals()[name]
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    with pytest.raises(amg.Refused) as e:
        agn.transfer_device(dA, dev(X), block_size=bs)
    assert (e.value.rule, e.value.row) == ("candidate", row)
    with pytest.raises(amg.Refused) as e:
        agn.sa_hierarchy(A, DEV, B=X, block_size=bs, max_coarse=2)
    assert (e.value.rule, e.value.row) == ("candidate", row)


def test_a_refused_node_block_reports_block_size_times_the_node():
    A, bs, X = NC.cases()["elasticity8_rbm"]
    agg = R.transfer(A, X, bs=bs)[3]["agg"]
    bad = X.copy()
    bad[:, 2] = np.where(np.repeat(agg, 2) == agg.max(), bad[:, 0], bad[:, 2])
    with pytest.raises(R.Refused) as want:
        R.transfer(A, bad, bs=bs)
    with pytest.raises(amg.Refused) as e:
        agn.transfer_device(ops.DeviceCSR.from_scipy(A, DEV), dev(bad), block_size=bs)
    assert (e.value.rule, e.value.row) == ("candidate", want.value.row) and want.value.row % 2 == 0 and want.value.row > 0
    # a looser rank_tol than a pivot ratio of a healthy aggregate refuses it as well: the keyword reaches the kernel
    with pytest.raises(amg.Refused):
        agn.transfer_device(ops.DeviceCSR.from_scipy(A, DEV), dev(X), block_size=bs, rank_tol=0.5)


# ---- the unchanged path ---------------------------------------------------------------------------------------------------------
def test_one_candidate_on_block_size_1_is_todays_path():
    A, _ = SC.problems()["jittered"]
    w = SC.wavy(A.shape[0])
    Ps, As, infos = sa_ref.sa_transfers(A, B=w, **SC.SA_KW)
    H1 = agn.sa_hierarchy(A, DEV, B=w, **SC.SA_KW)
    H2 = agn.sa_hierarchy(A, DEV, B=w.reshape(-1, 1), **SC.SA_KW)
    assert H1.sizes == H2.sizes == [M.shape[0] for M in As]
    for l1, l2, Pt in zip(H1.levels, H2.levels, Ps):
        assert_same(l1.P, l2.P, "P")
        assert_csr_equal(l1.P, Pt, "P against sa_ref")
    assert H1.amg_info == H2.amg_info
    assert [(d["block_size"], d["candidates"]) for d in H1.amg_info[:len(infos)]] == [(1, 1)] * len(infos)


# ---- a whole hierarchy ----------------------------------------------------------------------------------------------------------
KW = dict(block_size=2, max_coarse=50)
SOLVE = dict(smoother="Jacobi", smooth_steps=NC.STEPS, omega=NC.OMEGA, smoother_semantics="as_named")
CYCLES = 20


def deviation(got, want, largest):
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / (RTOL * np.abs(want) + FLOOR * largest)))


@functools.lru_cache(maxsize=None)
def solver():
    A, b, B, _ = NC.elasticity(16)
    return SmoothedAggregationAMG(A, b.reshape(-1, 1).copy(), B=B, **KW)


def test_whole_hierarchy_is_the_twins_and_cycles_as_the_oracle():
    A, b, B, _ = NC.elasticity(16)
    Ps, As, infos = NC.twin_hierarchy("rbm", max_coarse=50)
    assert [M.shape[0] for M in As] == [578, 84, 6]
    want = SC.oracle_history(A, b, Ps, cap=CYCLES, omega=NC.OMEGA, target=0.0)
    mg = solver()
    mg.solve(max_iterations=CYCLES + 1, error=0.0, **SOLVE)
    assert mg.level_dims == [578, 84, 6]
    for lev, Pt in zip(mg._hier.levels, Ps):
        assert_csr_equal(lev.P, Pt, "P")
    got = mg.get_track_res().ravel()
    assert got.size == len(want) == CYCLES + 1
    print("levels %s, %d cycles to %.2e ||b||, deviation %.3f of the bound"
          % (mg.level_dims, CYCLES, got[-1] / want[0], deviation(got[1:], want[1:], want[0])))
    assert deviation(got[1:], want[1:], want[0]) <= 1.0
    info = mg.hierarchy_info()
    assert [(d["n"], d["nnz"]) for d in info["levels"]] == [(M.shape[0], M.nnz) for M in As]
    assert info["levels"][:2] == infos and info["levels"][2] == {"n": 6, "nnz": As[2].nnz, "n_agg": None, "rounds": None}
    assert [(d["n_agg"], d["block_size"], d["candidates"]) for d in info["levels"][:2]] == [(28, 2, 3), (2, 3, 3)]
    assert info["operator_complexity"] == sum(M.nnz for M in As) / As[0].nnz


def test_translations_are_the_default_of_a_block_size():
    A, b, _, _ = NC.elasticity(16)
    Ps, As, infos = NC.twin_hierarchy("translations")
    H = agn.sa_hierarchy(A, DEV, block_size=2, max_coarse=100)
    assert H.sizes == [578, 56] and H.amg_info[0] == infos[0]
    assert_csr_equal(H.levels[0].P, Ps[0], "P")


def test_as_a_preconditioner_of_cg_and_gmres():
    """CG preconditioned by V(2,2) damped Jacobi 0.5 on elasticity_2d(16), max_coarse=100, to 1e-8 ||b||: the twin's count
    (tests/test_sa_block_cpu.py: 20 with the rigid-body modes), and more with today's vector of ones (58 there)."""
    A, b, B, _ = NC.elasticity(16)
    nb = np.linalg.norm(b)
    kw = dict(precond_steps=NC.STEPS, precond_omega=NC.OMEGA)
    counts = {}
    for which, setup in (("rbm", dict(B=B, block_size=2)), ("ones", dict())):
        H = agn.sa_hierarchy(A, DEV, max_coarse=100, **setup)
        assert H.sizes == [M.shape[0] for M in NC.twin_hierarchy(which)[1]]
        cg = CG(A, b.reshape(-1, 1).copy())
        cg.solve(max_iterations=200, error=NC.TARGET * nb, preconditioner=H, **kw)
        assert cg.get_residual() <= NC.TARGET * nb
        assert np.linalg.norm(b - A @ cg.get_solution().ravel()) <= 2 * NC.TARGET * nb
        counts[which] = cg.get_iterations()
        if which == "rbm":
            rbm = H
    print("CG iterations", counts, "the twin's", {w: NC.cg_iterations(w) for w in counts})
    assert counts["rbm"] == NC.cg_iterations("rbm") == 20
    assert counts["ones"] > counts["rbm"]
    g = GMRES(A, b.reshape(-1, 1).copy())
    g.solve(max_iterations=60, error=NC.TARGET * nb, restart=20, preconditioner=rbm, precond_cycle_shape="K",
            precond_k_inner="fcg", **kw)
    print("GMRES(20) with K-cycles: %d iterations" % g.get_iterations())
    assert g.get_residual() <= NC.TARGET * nb and np.linalg.norm(b - A @ g.get_solution().ravel()) <= 2 * NC.TARGET * nb
    Bs = b.reshape(-1, 1) * np.array([1.0, 2.0, -0.5])
    Xs, _ = CG(A, b.reshape(-1, 1).copy()).solve_many(Bs, max_iterations=60, error=NC.TARGET * nb * 0.5, preconditioner=rbm, **kw)
    for j in range(3):
        assert np.linalg.norm(Bs[:, j] - A @ Xs[:, j]) <= 2 * NC.TARGET * nb
