"""The Chebyshev polynomial smoother on the GPU (-m gpu): the tiled passes of csrc/stencil_tile.hip and csrc/dia_tile.hip
against the two-launch path (residual launch + lmg_cheby_update) and against the CPU twin (tests/chebyshev_ref.py), bit for
bit; whole solves against the twin's cycles; graph replay against eager launches; multigrid-preconditioned CG."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import chebyshev_ref as C                                            # noqa: E402  (checker only)
from fused_checks import (check_plain, check_transfers, cheby_histories as _histories,      # noqa: E402
                          cheby_knobs as knobs, cheby_twin_history as _twin_history, two_launch)
from learnmultigrid_amd import ops, problems as P                    # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy, chebyshev_coefficients   # noqa: E402
from oracle import kernels as K                                      # noqa: E402  (checker only)
from support import DEV, dev, nan_vec, operators                     # noqa: E402


def gershgorin_on_device(A, dA):
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    ops.csr_gershgorin(dA, out)
    g = float(out.item())
    assert g == C.gershgorin(A)                        # storage-order sums, one division, one maximum: the same bits
    return g


# 5-point at 257^2 and 1025^2, ragged widths (no multiple of a tile's inner part; 99: less than two tiles wide), 9-point
# Galerkin levels
GRIDS = [(257, "5pt"), (1025, "5pt"), (99, "5pt"), (771, "5pt"), (99, "9pt"), (513, "9pt"), (771, "9pt")]


@pytest.mark.parametrize("side,kind", GRIDS)
def test_tiled_pass_equals_two_launch_path_and_twin(side, kind):
    A, Pm, Rm = operators(side, kind)
    dA, dP, dR = (ops.DeviceCSR.from_scipy(M, DEV) for M in (A, Pm, Rm))
    for d_ in (dA, dP, dR):
        d_.pack()
    assert ops._cheby_kind(dA) == "tile" and ops.stencil_cheby_available(dA)
    assert ops.stencil_cheby_prolong_available(dA, dP) and ops.stencil_cheby_restrict_available(dA, dR)
    lmax = gershgorin_on_device(A, dA)
    if kind == "5pt":
        assert lmax == 2.0
    rng = np.random.default_rng(side)
    n, nc = A.shape[0], Pm.shape[1]
    x0, b, e = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(nc)
    for rows in (16, 32):
        with knobs(tile_rows=rows, tile_rows_big=rows):
            check_plain(A, dA, x0, b, lmax)
    check_plain(A, dA, x0, b, 1.7, ratio=9.0)                        # overridden bounds
    for hx in (1, 0):                                                # hot transfers on and off
        for layout in (dict(tile_rows=16, tile_rows_big=16), dict(tile_rows=32, tile_rows_big=32, tile_prol_wide_lines_hx=1 << 30),
                       dict(tile_rows=32, tile_rows_big=32, tile_prol_wide_lines_hx=0)):
            with knobs(tile_hot_transfers=hx, **layout):
                check_transfers(A, Pm, Rm, dA, dP, dR, x0, b, e, lmax)


def test_transfer_passes_through_the_pattern_tables():
    """No frequent pattern of R / pair of P: every coarse row and every correction through the pattern table."""
    A, Pm, Rm = operators(99, "9pt")
    dA, dP, dR = (ops.DeviceCSR.from_scipy(M, DEV) for M in (A, Pm, Rm))
    for d_ in (dA, dP, dR):
        d_.pack()
    rng = np.random.default_rng(99)
    n, nc = A.shape[0], Pm.shape[1]
    x0, b, e = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(nc)
    TR, TP = dR.restrict, dP.prolong
    hot, pairs = TR.hot, (TP._hot_pairs[0], TP._hot_pairs[1])
    try:
        TR.hot = -1
        TP._hot_pairs[0] = TP._hot_pairs[1] = -1
        check_transfers(A, Pm, Rm, dA, dP, dR, x0, b, e, C.gershgorin(A))
    finally:
        TR.hot = hot
        TP._hot_pairs[0], TP._hot_pairs[1] = pairs


@pytest.mark.parametrize("ne", [4096, 8191])
def test_one_dimensional_operator_runs_the_two_launch_path(ne):
    A = K.as_csr(P.poisson_1d_fd(ne)[0])
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack()
    assert not ops.stencil_cheby_available(dA)                       # no tiled pass for the 1-D slot set
    lmax = gershgorin_on_device(A, dA)
    rng = np.random.default_rng(ne)
    n = A.shape[0]
    x0, b = rng.standard_normal(n), rng.standard_normal(n)
    for S in (1, 2, 3, 5):
        coef = chebyshev_coefficients(lmax, 4.0, S)
        assert np.array_equal(two_launch(dA, x0, b, coef), C.cheby_step(A, x0, b, coef)), S
        assert np.array_equal(two_launch(dA, None, b, coef), C.cheby_step(A, np.zeros(n), b, coef)), S
    with pytest.raises(ops.LmgError):
        ops.stencil_cheby(dA, dev(x0), dev(b), chebyshev_coefficients(lmax, 4.0, 2), nan_vec(n))


def dia_matrix(name):
    if name == "varcoeff5_151":
        return K.as_csr(P.variable_coeff_poisson_2d_structured(150, seed=44)[0])
    if name == "jittered7_151":
        return K.as_csr(P.jittered_poisson_2d(150, seed=42)[0])
    if name == "jittered7_300x":
        return K.as_csr(P.jittered_poisson_2d(299, seed=7)[0])
    if name == "perturbed9_129":
        A = P.poisson_2d_structured(256)[0]
        Pm = P.tensor_interpolator_2d(257)
        G = sp.csr_matrix(Pm.T @ A @ Pm)
        G.sort_indices()
        rng = np.random.default_rng(3)
        G.data = G.data * (1.0 + 0.1 * rng.random(G.nnz))            # 9-point, every value distinct
        return K.as_csr(G)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["varcoeff5_151", "jittered7_151", "jittered7_300x", "perturbed9_129"])
@pytest.mark.parametrize("rows", [32, 64])
def test_dia_pass_equals_two_launch_path_and_twin(name, rows):
    A = dia_matrix(name)
    n = A.shape[0]
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack()
    assert dA.stencil is None and dA.dia is not None and ops._cheby_kind(dA) == "dia"
    lmax = gershgorin_on_device(A, dA)
    rng = np.random.default_rng(77)
    x0, b = rng.standard_normal(n), rng.standard_normal(n)
    with knobs(dia_rows=rows):
        check_plain(A, dA, x0, b, lmax)
    with pytest.raises(ops.LmgError):
        ops.stencil_cheby(dA, dev(x0), dev(b), chebyshev_coefficients(lmax, 4.0, 2), nan_vec(n), prolong=(None, None))


def test_entry_points_check_their_arguments():
    A, Pm, Rm = operators(99, "5pt")
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack()
    n = A.shape[0]
    x, b, out = dev(np.ones(n)), dev(np.ones(n)), nan_vec(n)
    for bad in ([], [(0.0, 1.0)] * 4):
        with pytest.raises(ops.LmgError):
            ops.stencil_cheby(dA, x, b, bad, out)
    with pytest.raises(ops.LmgError):
        ops.stencil_cheby(dA, x, b, [(0.0, 1.0)], x)                 # x_out aliases x_in
    d = nan_vec(n)
    with pytest.raises(ops.LmgError):
        ops.cheby_update(0.0, 1.0, x, b, d, d, first=True)           # d aliases x
    with pytest.raises(ops.LmgError):
        ops.cheby_update(0.0, 1.0, x, b, d, out[1:], first=True)     # not 16-byte aligned / wrong length


# ---- whole solves -----------------------------------------------------------------------------------------------------------
def _problem(name):
    if name == "cfg2_513":
        A, rhs = P.poisson_2d_structured(512)
        return A, rhs, P.geometric_hierarchy_2d(513, 3)
    A, rhs = P.variable_coeff_poisson_2d_structured(256, seed=44)
    return A, rhs, P.geometric_hierarchy_2d(257, 3)


@pytest.mark.parametrize("name", ["cfg2_513", "varcoeff_257"])
def test_solve_histories_match_the_twin_and_graph_replay_matches_eager(name):
    A, rhs, hier = _problem(name)
    H = Hierarchy(A, hier, DEV)
    kinds = [ops._cheby_kind(lev.A) for lev in H.levels[:-1]]
    assert kinds == (["tile", "tile"] if name == "cfg2_513" else ["dia", "dia"]), kinds
    for degree, shape, cycles in ((3, "V", 6), (2, "W", 4), (5, "V", 4)):
        got, x = _histories(H, rhs, cycles, degree, shape)
        want, xw, ref = _twin_history(A, rhs, hier, cycles, degree, shape, H=H)
        assert H.cheby_key()[0] == tuple(ref.lmax)                                 # the Gershgorin bounds, bit for bit
        rel = np.abs(got - want) / want
        print("%s degree %d %s: history rel. diff max %.3e, reduction %.3e" % (name, degree, shape, rel.max(), got[-1] / got[0]))
        assert np.all(rel <= 1e-10), (name, degree, shape, rel)
        lu, _, _ = _twin_history(A, rhs, hier, cycles, degree, shape)            # (for the record: sparse LU on the coarsest level)
        print("    against the twin with a sparse LU: max |diff| / first residual %.3e" % (np.abs(got - lu).max() / lu[0]))
        gg, xg = _histories(H, rhs, cycles, degree, shape, graph=True)
        assert np.array_equal(gg, got) and np.array_equal(xg, x), (name, degree, shape, "graph replay vs eager")
    # degree 5 ran the two-launch path; degree 3 with the fused passes off runs it too and gives the same bits
    got, x = _histories(H, rhs, 3, 3)
    try:
        ops.set_fused_enabled(False)
        assert not any(ops.stencil_cheby_available(lev.A) for lev in H.levels[:-1])
        got2, x2 = _histories(H, rhs, 3, 3)
    finally:
        ops.set_fused_enabled(True)
    assert np.array_equal(got, got2) and np.array_equal(x, x2)


def test_graph_key_carries_the_bounds():
    A, rhs, hier = _problem("cfg2_513")
    H = Hierarchy(A, hier, DEV)
    with torch.cuda.stream(H.stream):
        g1 = H.captured_cycle("Chebyshev", 3, 1.0, "lexicographic")
        g2 = H.captured_cycle("Chebyshev", 3, 1.0, "lexicographic")
        g3 = H.captured_cycle("Chebyshev", 3, 1.0, "lexicographic", cheby_lmax=1.9, cheby_ratio=6.0)
        g4 = H.captured_cycle("Chebyshev", 3, 1.0, "lexicographic", cheby_ratio=4.0)
    assert g1 is g2 and g3 is not g1 and g4 is g1


def test_solver_front_end():
    from learnmultigrid_amd.solvers import HierarchyMG
    A, rhs, hier = _problem("cfg2_513")
    kw = dict(levels=3, smooth_steps=3, max_iterations=12, error=1e-8)
    tracks = {}
    for graph in (False, True):
        mg = HierarchyMG(A, rhs.copy(), hier)
        mg.solve(smoother="Chebyshev", smoother_semantics="as_named", use_graph=graph, **kw)
        tracks[graph] = mg.get_track_res().copy()
    assert np.array_equal(tracks[False], tracks[True])
    # track[0] is the reference's ||1||; track[k] the residual after k cycles
    want, _, _ = _twin_history(A, rhs, hier, len(tracks[True]) - 1, 3, H=mg._hier)
    np.testing.assert_allclose(tracks[True][1:, 0], want[1:], rtol=1e-10, atol=0)
    assert tracks[True][-1, 0] <= 1e-8
    # as shipped the name is ignored: forward Gauss-Seidel runs
    kw2 = dict(levels=3, smooth_steps=1, max_iterations=3, error=1e-8)
    a = HierarchyMG(A, rhs.copy(), hier)
    a.solve(smoother="Chebyshev", **kw2)
    g = HierarchyMG(A, rhs.copy(), hier)
    g.solve(smoother="GaussSeidel", **kw2)
    assert np.array_equal(a.get_track_res(), g.get_track_res())
    with pytest.raises(ValueError):
        HierarchyMG(A, rhs.copy(), hier).solve(smoother="Chebyshev", smoother_semantics="as_named", cheby_ratio=1.0, **kw)
    # one cycle through v_cycle / w_cycle
    mg = HierarchyMG(A, rhs.copy(), hier)
    ref = C.ChebyCycle.galerkin(A, hier)
    for fn, shape in ((mg.v_cycle, "V"), (mg.w_cycle, "W"), (mg.f_cycle, "F")):
        u = fn(mg.matrix, np.zeros((A.shape[0], 1)), rhs, "Chebyshev", 3, 1e-8, 3, first_call=True, smoother_semantics="as_named")
        w = ref.cycle(np.zeros(A.shape[0]), rhs.ravel(), degree=3, shape=shape)
        np.testing.assert_allclose(u.ravel(), w, rtol=0, atol=1e-10 * np.abs(w).max())


def test_torch_ops():
    ops.register_torch_ops()
    A = K.as_csr(P.poisson_2d_structured(128)[0])
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    h = torch.ops.lmg.operator_create(dA.rowptr, dA.colidx, dA.vals, A.shape[1])
    try:
        assert float(torch.ops.lmg.operator_gershgorin(h).item()) == 2.0
        assert float(torch.ops.lmg.csr_gershgorin(dA.rowptr, dA.colidx, dA.vals).item()) == 2.0
        rng = np.random.default_rng(1)
        x0, b = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
        for S in (2, 5):
            got = torch.ops.lmg.operator_chebyshev(h, dev(x0), dev(b), S, 0.0, 4.0).cpu().numpy()
            assert np.array_equal(got, C.cheby_step(A, x0, b, C.coefficients(2.0, 4.0, S)))
    finally:
        torch.ops.lmg.operator_free(h)


# ---- preconditioned CG ------------------------------------------------------------------------------------------------------
def test_mg_pcg_with_the_chebyshev_cycle():
    from learnmultigrid_amd.solvers import CG
    A, rhs, hier = _problem("cfg2_513")
    H = Hierarchy(A, hier, DEV)
    its = {}
    for steps in (2, 3):
        for sm in ("Chebyshev", "Jacobi"):
            cg = CG(A, rhs.copy())
            cg.solve(max_iterations=200, error=1e-8, preconditioner=H, precond_smoother=sm, precond_steps=steps)
            assert cg.get_track_res()[-1, 0] <= 1e-8, (sm, steps)
            its[sm, steps] = cg.get_iterations()
        print("MG-PCG cfg#2, %d steps: Chebyshev %d iterations, Jacobi(0.8) %d" % (steps, its["Chebyshev", steps], its["Jacobi", steps]))
        assert its["Chebyshev", steps] <= its["Jacobi", steps]


def symmetric_form(A):
    """The operator with the couplings of interior rows to the Dirichlet (identity) rows dropped: its symmetric interior
    block next to an identity -- the same problem for zero boundary data."""
    A = K.as_csr(A)
    bnd = np.diff(A.indptr) == 1
    coo = A.tocoo()
    keep = ~(bnd[coo.col] & (coo.row != coo.col))
    out = K.as_csr(sp.csr_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), shape=A.shape))
    assert abs(out - out.T).max() == 0.0
    return out


def test_the_chebyshev_cycle_is_a_symmetric_operator():
    """M = one cycle from a zero iterate.  A polynomial in D^-1 A applied to D^-1 is symmetric when A is, and with R = P^T,
    Galerkin coarse operators and the direct coarse solve so is the cycle.  cfg#2 as assembled is NOT a symmetric matrix
    (its Dirichlet rows are identity rows whose columns the interior rows still reference; with it <Mu, v> and <u, Mv> differ
    by 1.7e-6 relative), so the check runs on its symmetric form: same grid, transfers and levels."""
    A, rhs, hier = _problem("cfg2_513")
    A = symmetric_form(A)
    H = Hierarchy(A, hier, DEV)
    assert [ops._cheby_kind(lev.A) for lev in H.levels[:-1]] == ["tile", "tile"]
    rng = np.random.default_rng(2024)
    n = A.shape[0]
    u, v = rng.random(n), rng.random(n)

    def M(w, degree, shape):
        with torch.cuda.stream(H.stream):
            H.levels[0].b.copy_(dev(w))
            H.cycle("Chebyshev", degree, x_is_zero=True, shape=shape)
            return H.levels[0].x.cpu().numpy().copy()

    for degree, shape in ((2, "V"), (3, "V"), (3, "W")):
        a, b = float(np.dot(M(u, degree, shape), v)), float(np.dot(u, M(v, degree, shape)))
        print("degree %d %s: <Mu, v> = %.17g, <u, Mv> = %.17g, rel. diff %.3e" % (degree, shape, a, b, abs(a - b) / abs(a)))
        assert abs(a - b) <= 1e-12 * abs(a)
