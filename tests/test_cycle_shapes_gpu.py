"""W- and F-cycles (-m gpu): the turnaround pass of stencil_tile.hip (lmg_stencil_smooth_tiled_turnaround) bitwise
against the two passes it replaces and against the oracle, under every tile forcing; cycle histories against the CPU
restatement of pyamg's cycle shapes (cycle_shapes_ref.ShapeCycle); the solver keywords."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from learnmultigrid_amd import ops, problems as P    # noqa: E402
from learnmultigrid_amd._lib import LmgError         # noqa: E402
from oracle import kernels as K                      # noqa: E402  (checker only)
from cycle_shapes_ref import ShapeCycle, history     # noqa: E402  (checker only)
from fused_checks import knobs_over                  # noqa: E402
from support import DEV, dev, operators              # noqa: E402

KNOBS = ("tile_hot_transfers", "tile_rows", "tile_rows_big", "tile_turnaround_rows")
knobs = knobs_over(KNOBS)
PAIRS = [(a, b) for a in (1, 2, 3) for b in (1, 2, 3)]


def packed(A, Pm, Rm):
    dA, dP, dR = (ops.DeviceCSR.from_scipy(M, DEV) for M in (A, Pm, Rm))
    for d in (dA, dP, dR):
        d.pack()
    assert ops.stencil_smooth_turnaround_available(dA, dP, dR)
    return dA, dP, dR


def check_turnaround(A, Pm, Rm, dA, dP, dR, x0, b, e, pairs=PAIRS):
    """(a) the correcting pass then the restricting pass, (b) the oracle: x + P e, s_post + s_pre sweeps, R (b - A x)."""
    n, nc = A.shape[0], Pm.shape[1]
    dx, db, de = dev(x0), dev(b), dev(e)
    for sp_, sr in pairs:
        want = K.spmv(Pm, e, x0.copy(), 1.0, 1.0)
        for _ in range(sp_ + sr):
            want = K.jacobi(A, want, b, 0.8)
        wbc = K.matvec(Rm, K.residual(A, want, b)[0])
        y = torch.full((n,), np.nan, dtype=torch.float64, device=DEV)
        z, out = torch.full_like(y, np.nan), torch.full_like(y, np.nan)
        bc1 = torch.full((nc,), np.nan, dtype=torch.float64, device=DEV)
        bc2 = torch.full_like(bc1, np.nan)
        ops.stencil_smooth(dA, dx, db, 0.8, sp_, y, None, prolong=(dP, de))
        ops.stencil_smooth(dA, y, db, 0.8, sr, z, None, restrict=(dR, bc1))
        ops.stencil_smooth_turnaround(dA, dx, db, 0.8, sp_, sr, out, prolong=(dP, de), restrict=(dR, bc2))
        got, gbc = out.cpu().numpy(), bc2.cpu().numpy()
        assert np.array_equal(got, z.cpu().numpy()), (n, sp_, sr, np.flatnonzero(got != z.cpu().numpy())[:8])
        assert np.array_equal(gbc, bc1.cpu().numpy()), (n, sp_, sr)
        assert np.array_equal(got, want), (n, sp_, sr)
        assert np.array_equal(gbc, wbc), (n, sp_, sr, np.flatnonzero(gbc != wbc)[:8])


def _data(A, Pm, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0]), rng.standard_normal(Pm.shape[1])


@pytest.fixture(scope="module")
def level1():
    """Level 1 of cfg#4: the 2049^2 9-point Galerkin operator and the transfers to 1025^2."""
    A, Pm, Rm = operators(2049, "9pt")
    return (A, Pm, Rm) + packed(A, Pm, Rm) + _data(A, Pm, 2049)


def test_level1_turnaround_every_sweep_pair(level1):
    A, Pm, Rm, dA, dP, dR, x0, b, e = level1
    assert dR.restrict.hot >= 0 and min(dP.prolong._hot_pairs) >= 0
    check_turnaround(A, Pm, Rm, dA, dP, dR, x0, b, e)


@pytest.mark.parametrize("rows", [32, 64])
@pytest.mark.parametrize("hx", [0, 1])
def test_level1_turnaround_every_layout(level1, rows, hx):
    A, Pm, Rm, dA, dP, dR, x0, b, e = level1
    with knobs(tile_turnaround_rows=rows, tile_hot_transfers=hx):
        check_turnaround(A, Pm, Rm, dA, dP, dR, x0, b, e, pairs=[(3, 3), (1, 2)])


# odd and uneven sizes, widths that are no multiple of a tile's inner part, 65 / 99 columns (less than two tiles wide)
CASES = [(65, "5pt"), (65, "9pt"), (99, "5pt"), (99, "9pt"), (257, "9pt"), (769, "5pt"), (769, "9pt"), (1029, "9pt"),
         (1537, "5pt")]
LAYOUTS = [dict(tile_turnaround_rows=r, tile_hot_transfers=h, tile_rows=t, tile_rows_big=t)
           for r in (0, 32, 64) for h in (0, 1) for t in (16, 32)]


@pytest.mark.parametrize("side,kind", CASES)
def test_turnaround_on_small_grids(side, kind):
    A, Pm, Rm = operators(side, kind)
    dA, dP, dR = packed(A, Pm, Rm)
    x0, b, e = _data(A, Pm, side)
    for i, layout in enumerate(LAYOUTS):
        with knobs(**layout):
            check_turnaround(A, Pm, Rm, dA, dP, dR, x0, b, e, pairs=PAIRS if (side <= 257 or i == 0) else [(3, 3), (2, 1)])


@pytest.mark.parametrize("side,kind", [(99, "9pt"), (769, "9pt"), (1029, "5pt")])
def test_turnaround_through_the_pattern_tables(side, kind):
    """No frequent pattern of R / pair of P: every coarse row and every correction through the pattern table."""
    A, Pm, Rm = operators(side, kind)
    dA, dP, dR = packed(A, Pm, Rm)
    x0, b, e = _data(A, Pm, side + 1)
    TR, TP = dR.restrict, dP.prolong
    hot, pairs = TR.hot, (TP._hot_pairs[0], TP._hot_pairs[1])
    try:
        TR.hot = -1
        TP._hot_pairs[0] = TP._hot_pairs[1] = -1
        for rows in (32, 64):
            with knobs(tile_turnaround_rows=rows, tile_hot_transfers=1):
                check_turnaround(A, Pm, Rm, dA, dP, dR, x0, b, e, pairs=[(3, 3), (1, 1)])
    finally:
        TR.hot = hot
        TP._hot_pairs[0], TP._hot_pairs[1] = pairs


def test_turnaround_arguments_and_switches():
    A, Pm, Rm = operators(99, "9pt")
    dA, dP, dR = packed(A, Pm, Rm)
    n, nc = A.shape[0], Pm.shape[1]
    x, b, out = (torch.zeros(n, dtype=torch.float64, device=DEV) for _ in range(3))
    e, bc = torch.zeros(nc, dtype=torch.float64, device=DEV), torch.zeros(nc, dtype=torch.float64, device=DEV)
    with pytest.raises(LmgError):            # the single pass keeps rejecting both transfers
        ops.stencil_smooth(dA, x, b, 0.8, 3, out, None, prolong=(dP, e), restrict=(dR, bc))
    for bad in ((0, 3), (3, 4)):
        with pytest.raises(LmgError):
            ops.stencil_smooth_turnaround(dA, x, b, 0.8, bad[0], bad[1], out, prolong=(dP, e), restrict=(dR, bc))
    with pytest.raises(LmgError):            # b_coarse aliasing e
        ops.stencil_smooth_turnaround(dA, x, b, 0.8, 1, 1, out, prolong=(dP, e), restrict=(dR, e))
    with pytest.raises(LmgError):
        ops.tune_set("tile_turnaround_rows", 48)
    ops.set_fused_turnaround_enabled(False)
    try:
        assert not ops.stencil_smooth_turnaround_available(dA, dP, dR)
    finally:
        ops.set_fused_turnaround_enabled(True)
    assert ops.stencil_smooth_turnaround_available(dA, dP, dR)


# ---- cycles ------------------------------------------------------------------------------------------------------
def _solve(A, rhs, hier, its, shape, graph=False, turnaround=True, **kw):
    """turnaround: True (the default selection), False (never), "all" (on every level where the pass can run)."""
    from learnmultigrid_amd.solvers import HierarchyMG
    window = ops.TURNAROUND_MIN_ROWS, ops.TURNAROUND_MAX_ROWS
    ops.set_fused_turnaround_enabled(bool(turnaround))
    if turnaround == "all":
        ops.TURNAROUND_MIN_ROWS, ops.TURNAROUND_MAX_ROWS = 0, 1 << 62
    try:
        mg = HierarchyMG(A, rhs.copy(), hier)
        mg.solve(levels=len(hier) + 1, smooth_steps=3, max_iterations=its, error=1e-30, cycle_shape=shape,
                 use_graph=graph, **kw)
    finally:
        ops.set_fused_turnaround_enabled(True)
        ops.TURNAROUND_MIN_ROWS, ops.TURNAROUND_MAX_ROWS = window
    return mg


def _compare(mg, A, rhs, hier, its, shape, gs_sweep=("forward", "forward"), **kw):
    want, _ = history(ShapeCycle(A, hier, shape, gs_sweep), A, rhs, its, **kw)
    got = mg.get_track_res().ravel()
    assert got.shape == want.shape
    assert got[0] == np.sqrt(float(A.shape[0]))
    np.testing.assert_allclose(got[1:], want[1:], rtol=1e-10, atol=1e-14 * want.max())


def _bitwise(a, b):
    assert np.array_equal(a.get_track_res(), b.get_track_res())
    assert np.array_equal(a.get_solution(), b.get_solution())


JAC = dict(smoother="Jacobi", smoother_semantics="as_named", omega=0.8)


def test_cfg4_w_cycle_history():
    """cfg#4 (4097^2, 6 levels) W(3,3) weighted Jacobi over 5 cycles; turnaround on / off and graph replay bitwise."""
    m, levels, its = 4096, 6, 5
    A, rhs = P.poisson_2d_structured(m)
    hier = P.geometric_hierarchy_2d(m + 1, levels)
    mg = _solve(A, rhs, hier, its, "W", **JAC)
    _compare(mg, A, rhs, hier, its, "W", smoother="Jacobi", steps=3, omega=0.8)
    _bitwise(mg, _solve(A, rhs, hier, its, "W", turnaround=False, **JAC))
    _bitwise(mg, _solve(A, rhs, hier, its, "W", turnaround="all", **JAC))
    _bitwise(mg, _solve(A, rhs, hier, its, "W", graph=True, **JAC))
    _bitwise(mg, _solve(A, rhs, hier, its, "W", graph=True, turnaround="all", **JAC))
    v = _solve(A, rhs, hier, its, "V", **JAC)
    assert mg.get_track_res()[-1, 0] < v.get_track_res()[-1, 0]


@pytest.mark.parametrize("levels", [3, 5])
def test_cfg2_f_cycle_history(levels):
    m, its = 512, 6
    A, rhs = P.poisson_2d_structured(m)
    hier = P.geometric_hierarchy_2d(m + 1, levels)
    mg = _solve(A, rhs, hier, its, "F", turnaround="all", **JAC)
    _compare(mg, A, rhs, hier, its, "F", smoother="Jacobi", steps=3, omega=0.8)
    _bitwise(mg, _solve(A, rhs, hier, its, "F", turnaround=False, **JAC))
    _bitwise(mg, _solve(A, rhs, hier, its, "F", **JAC))
    _bitwise(mg, _solve(A, rhs, hier, its, "F", graph=True, turnaround="all", **JAC))
    w = _solve(A, rhs, hier, its, "W", turnaround="all", **JAC)
    _compare(w, A, rhs, hier, its, "W", smoother="Jacobi", steps=3, omega=0.8)
    _bitwise(w, _solve(A, rhs, hier, its, "W", graph=True, turnaround="all", **JAC))
    _bitwise(w, _solve(A, rhs, hier, its, "W", graph=True, turnaround=False, **JAC))


def test_default_turnaround_selection_follows_the_measurements():
    """cfg#4: the turnaround runs on 1025^2 and 513^2 (measured faster), not on 2049^2 or 257^2 (measured slower)."""
    from learnmultigrid_amd.hierarchy import Hierarchy
    m, levels = 4096, 6
    A, _ = P.poisson_2d_structured(m)
    H = Hierarchy(A, P.geometric_hierarchy_2d(m + 1, levels), DEV)
    got = [ops.stencil_smooth_turnaround_selected(lev.A, lev.P, lev.R) for lev in H.levels[:-1]]
    assert got == [False, False, True, True, False]
    assert [ops.stencil_smooth_turnaround_available(lev.A, lev.P, lev.R) for lev in H.levels[:-1]] == \
        [False, True, True, True, True]


@pytest.mark.parametrize("shape", ["W", "F"])
def test_learned_like_hierarchy(shape):
    """Row-stochastic perturbed transfers: no level runs the fused transfers; steps = 4 splits every smoothing half."""
    m, levels, its = 256, 4, 4
    A, rhs = P.poisson_2d_structured(m)
    hier = [P.learned_like(Q, seed=7 + i) for i, Q in enumerate(P.geometric_hierarchy_2d(m + 1, levels))]
    mg = _solve(A, rhs, hier, its, shape, turnaround="all", **JAC)
    _compare(mg, A, rhs, hier, its, shape, smoother="Jacobi", steps=3, omega=0.8)
    _bitwise(mg, _solve(A, rhs, hier, its, shape, graph=True, turnaround="all", **JAC))
    from learnmultigrid_amd.solvers import HierarchyMG
    g = HierarchyMG(A, rhs.copy(), hier)
    g.solve(levels=levels, smooth_steps=4, max_iterations=its, error=1e-30, cycle_shape=shape, **JAC)
    _compare(g, A, rhs, hier, its, shape, smoother="Jacobi", steps=4, omega=0.8)


@pytest.mark.parametrize("shape", ["W", "F"])
@pytest.mark.parametrize("gs_sweep", ["forward", ("forward", "backward")], ids=["fwd", "fwd_bwd"])
def test_gauss_seidel_as_shipped(shape, gs_sweep):
    m, levels, its = 512, 4, 4
    A, rhs = P.poisson_2d_structured(m)
    hier = P.geometric_hierarchy_2d(m + 1, levels)
    mg = _solve(A, rhs, hier, its, shape, smoother="Jacobi", gs_sweep=gs_sweep)       # as_shipped: Gauss-Seidel
    _compare(mg, A, rhs, hier, its, shape, gs_sweep, smoother="GaussSeidel", steps=3)
    _bitwise(mg, _solve(A, rhs, hier, its, shape, graph=True, smoother="Jacobi", gs_sweep=gs_sweep))


def test_solver_keywords_and_single_cycles():
    from learnmultigrid_amd.solvers import GeometricMG, HierarchyMG
    m, levels = 128, 4
    A, rhs = P.poisson_2d_structured(m)
    hier = P.geometric_hierarchy_2d(m + 1, levels)
    mg = HierarchyMG(A, rhs.copy(), hier)
    with pytest.raises(ValueError):
        mg.solve(levels=levels, cycle="W")                   # the reference's V-only switch is kept
    with pytest.raises(ValueError):
        mg.solve(levels=levels, cycle_shape="X")
    rng = np.random.default_rng(3)
    u = rng.standard_normal((A.shape[0], 1))
    for name, shape in (("w_cycle", "W"), ("f_cycle", "F"), ("v_cycle", "V")):
        u0 = u.copy()
        out = getattr(mg, name)(A, u0, rhs, "Jacobi", 3, 1e-8, levels, smoother_semantics="as_named", omega=0.8)
        pre = u.ravel().copy()
        for _ in range(3):
            pre = K.jacobi(K.as_csr(A), pre, rhs.ravel(), 0.8)
        np.testing.assert_allclose(u0.ravel(), pre, rtol=1e-13, atol=1e-15 * np.abs(pre).max())   # pre-smoothed iterate
        want = ShapeCycle(A, hier, shape).cycle(u.ravel(), rhs.ravel(), "Jacobi", 3, 0.8)
        np.testing.assert_allclose(out.ravel(), want, rtol=1e-10, atol=1e-12 * np.abs(want).max())
    g = GeometricMG(*P.poisson_1d_fd(256))
    g.solve(levels=4, smoother="GaussSeidel", smooth_steps=2, max_iterations=30, error=1e-9, cycle_shape="W")
    assert g.get_track_res()[-1, 0] <= 1e-9


def _symmetric_problem(m=256):
    A, rhs = P.poisson_2d_structured(m)
    s = m + 1
    idx = np.arange(s * s)
    inter = ((idx % s) > 0) & ((idx % s) < m) & ((idx // s) > 0) & ((idx // s) < m)
    keep = sp.diags(inter.astype(float))
    As = sp.csr_matrix(keep @ A @ keep + sp.diags((~inter).astype(float)))
    return As, rhs, s


def test_w_cycle_preconditioned_cg():
    from learnmultigrid_amd.hierarchy import Hierarchy
    from learnmultigrid_amd.solvers import CG
    As, rhs, s = _symmetric_problem()
    H = Hierarchy(As, P.geometric_hierarchy_2d(s, 5), DEV)
    fine = H.levels[0]
    rng = np.random.default_rng(37)
    y, z = rng.standard_normal(As.shape[0]), rng.standard_normal(As.shape[0])

    def M(r, smoother, pair):
        fine.b.copy_(dev(r))
        H.cycle(smoother, 2, 0.8 if smoother == "Jacobi" else 1.0, x_is_zero=True, gs_sweep=pair, shape="W")
        return fine.x.cpu().numpy().copy()

    for smoother, pair in (("Jacobi", "forward"), ("GaussSeidel", ("forward", "backward"))):
        My, Mz = M(y, smoother, pair), M(z, smoother, pair)
        assert abs(y @ Mz - z @ My) <= 1e-12 * np.linalg.norm(y) * np.linalg.norm(Mz), smoother
    H.check_smoothers()
    ref = CG(As, rhs.copy())
    ref.solve(max_iterations=3000, error=1e-10)
    for smoother in ("Jacobi", "GaussSeidel"):
        cg = CG(As, rhs.copy())
        cg.solve(max_iterations=100, error=1e-10, preconditioner=H, precond_smoother=smoother, precond_cycle_shape="W")
        assert cg.get_track_res()[-1, 0] <= 1e-10, smoother
        x = ref.get_solution()
        assert np.linalg.norm(cg.get_solution() - x) <= 1e-6 * np.linalg.norm(x)
    with pytest.raises(ValueError):
        CG(As, rhs.copy()).solve(max_iterations=1, preconditioner=H, precond_cycle_shape="F")
