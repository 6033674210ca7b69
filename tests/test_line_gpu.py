"""The line relaxation smoother on the GPU (-m gpu): lmg_line_factor and lmg_line_solve (csrc/line.hip) against the CPU twin
(tests/line_ref.py) bit for bit, their flags and argument checks, whole solves against the twin's cycles, graph replay against
eager launches, the symmetry of the cycle, multigrid-preconditioned CG, rebuild_numeric and the torch.ops entries.

Shapes: system counts and lengths that are no multiples of 64 (65, 67, 131, 33), a single active lane in the last wave (65
systems; 130 systems as two colours of 65), odd line counts for zebra (67, 131, 33), W < 64 (40), lengths around the block
sizes of the kernels (test_short_systems)."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import line_ref as LR                                               # noqa: E402  (checker only)
from learnmultigrid_amd import _lib, ops, problems as P             # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy                  # noqa: E402
from oracle import kernels as K                                     # noqa: E402  (checker only)
from support import DEV, dev                                        # noqa: E402

GRIDS = [(65, 67), (40, 131), (130, 33)]                            # (W, H): line stride and number of lines


def _sub_grid(A, s, Wg, Hg):
    """The Wg x Hg corner of an operator on the s x s grid, renumbered with line stride Wg."""
    idx = (np.arange(Hg)[:, None] * s + np.arange(Wg)[None, :]).ravel()
    return K.as_csr(sp.csr_matrix(A)[idx][:, idx])


def _t1(n):
    return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))


def operator(kind, Wg, Hg):
    if kind == "aniso5":                                            # -(ax u_xx + ay u_yy), identity boundary rows
        A = sp.kron(sp.identity(Hg), 1e-3 * _t1(Wg)) + sp.kron(_t1(Hg), sp.identity(Wg))
        y, x = np.divmod(np.arange(Wg * Hg), Wg)
        bnd = (x == 0) | (x == Wg - 1) | (y == 0) | (y == Hg - 1)
        return K.as_csr(P.apply_dirichlet_identity_rows(A, np.zeros((Wg * Hg, 1)), bnd)[0])
    if kind == "galerkin9":                                         # P^T A P of the next finer grid
        Wf, Hf = 2 * Wg - 1, 2 * Hg - 1
        Af = operator("aniso5", Wf, Hf)
        Pf = sp.kron(P.geometric_interpolator_1d(Hf), P.geometric_interpolator_1d(Wf), format="csr")
        assert Pf.shape == (Wf * Hf, Wg * Hg)
        return K.as_csr(sp.csr_matrix(Pf.T @ Af @ Pf))
    s = max(Wg, Hg)
    if kind == "varcoeff5":
        return _sub_grid(P.variable_coeff_poisson_2d_structured(s - 1, seed=44)[0], s, Wg, Hg)
    if kind == "jittered7":
        return _sub_grid(P.jittered_poisson_2d(s - 1, seed=42)[0], s, Wg, Hg)
    raise KeyError(kind)


# ---- 1. the two entry points against the twin, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["aniso5", "galerkin9", "varcoeff5", "jittered7"])
@pytest.mark.parametrize("Wg,Hg", GRIDS)
def test_factor_and_solve_equal_the_twin_bit_for_bit(kind, Wg, Hg):
    A = operator(kind, Wg, Hg)
    n = A.shape[0]
    assert n == Wg * Hg
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    rng = np.random.default_rng(Wg * 1000 + Hg)
    x0, r0 = rng.standard_normal(n), rng.standard_normal(n)
    for d in "xy":
        want_fac, want_flags = LR.factor(A, Wg, d)
        fac, flags = ops.line_factor_flags(dA, Wg, d)
        assert flags == want_flags == 0, (kind, d, flags, want_flags)
        for name, g, w in zip(("lo", "minv", "cp"), fac, want_fac):
            g = g.cpu().numpy()
            assert np.array_equal(g, w), (kind, d, name, np.flatnonzero(g != w)[:8])
        for first, step in ((0, 1), (0, 2), (1, 2)):
            for omega in (1.0, 0.8):
                x, r = dev(x0), dev(r0)
                ops.line_solve(Wg, d, first, step, fac, r, omega, x)
                wx, wr = LR.solve(want_fac, Wg, d, first, step, r0, omega, x0)
                gx, gr = x.cpu().numpy(), r.cpu().numpy()
                assert np.array_equal(gx, wx), (kind, d, first, step, omega, np.flatnonzero(gx != wx)[:8])
                assert np.array_equal(gr, wr), (kind, d, first, step, omega, np.flatnonzero(gr != wr)[:8])
                # rows outside the selected systems keep their bits
                keep = np.ones(LR.by_system(x0, Wg, d).shape, dtype=bool)
                keep[first::step] = False
                assert np.array_equal(LR.by_system(gx, Wg, d)[keep], LR.by_system(x0, Wg, d)[keep])
                assert np.array_equal(LR.by_system(gr, Wg, d)[keep], LR.by_system(r0, Wg, d)[keep])
                assert keep.any() == (step == 2)


@pytest.mark.parametrize("Wg,Hg", [(3, 5), (9, 8), (32, 17), (33, 16), (34, 18), (64, 33), (65, 34)])
def test_short_systems(Wg, Hg):
    """Lengths around the kernels' block sizes: after the peeled first element a system goes in blocks of 32 (direction x) or
    16 (direction y) elements, what is left in blocks of 8, then element by element.  x lengths 3, 9, 32, 33 (one block), 34,
    64 (32 + 3 * 8 + 7), 65 (two blocks); y lengths 5, 8, 17 (one block), 16, 18, 33 (two blocks), 34."""
    A = operator("aniso5", Wg, Hg)
    n = A.shape[0]
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    rng = np.random.default_rng(Wg + Hg)
    x0, r0 = rng.standard_normal(n), rng.standard_normal(n)
    for d in "xy":
        want_fac, _ = LR.factor(A, Wg, d)
        fac = ops.line_factor(dA, Wg, d)
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(fac, want_fac))
        for first, step in ((0, 1), (1, 2), (2, 1000), (Wg + Hg, 1)):          # the last: no system at all, nothing changes
            x, r = dev(x0), dev(r0)
            ops.line_solve(Wg, d, first, step, fac, r, 0.8, x)
            wx, wr = LR.solve(want_fac, Wg, d, first, step, r0, 0.8, x0)
            assert np.array_equal(x.cpu().numpy(), wx) and np.array_equal(r.cpu().numpy(), wr), (d, first, step)


# ---- 2. flags and errors ----------------------------------------------------------------------------------------------------------
def helix(W, H):
    """The 5-point operator whose x-links run on across the line ends: row i couples to row i + 1 everywhere (what an
    x-periodic operator is in the linear row index)."""
    n = W * H
    return K.as_csr(sp.diags([-1.0, -1.0, 4.5, -1.0, -1.0], [-W, -1, 0, 1, W], shape=(n, n)).tocsr())


def test_flags():
    W = 33
    A = helix(W, W)
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    assert ops.line_factor_flags(dA, W, "x")[1] == ops.LINE_COUPLED == LR.factor(A, W, "x")[1]
    assert ops.line_factor_flags(dA, W, "y")[1] == 0
    with pytest.raises(ValueError, match="couples two x-lines"):
        ops.line_factor(dA, W, "x")
    hier = P.geometric_hierarchy_2d(W, 2)
    for bad in ("x", "xy"):
        with pytest.raises(ValueError, match=r"level 0.*couples two x-lines"):
            Hierarchy(A, hier, DEV).prepare_smoother("Line", line_dir=bad)
    H = Hierarchy(A, hier, DEV)
    with torch.cuda.stream(H.stream):
        H.prepare_smoother("Line", line_dir="y")
        H.levels[0].b.copy_(dev(np.ones(A.shape[0])))
        H.cycle("Line", 1, 1.0, x_is_zero=True)
        assert np.isfinite(H.residual_norm())
    # a stored zero in an identity row: a zero pivot in either direction
    Z = K.as_csr(P.poisson_2d_structured(W - 1)[0]).copy()
    Z.data[Z.indptr[4]] = 0.0
    dZ = ops.DeviceCSR.from_scipy(Z, DEV)
    for d in "xy":
        assert ops.line_factor_flags(dZ, W, d)[1] == ops.LINE_PIVOT == LR.factor(Z, W, d)[1]
        with pytest.raises(ValueError, match="pivot"):
            ops.line_factor(dZ, W, d)
    # a non-singular operator whose x-line 5 starts with the diagonal block [[1, 1], [1, 1]]: den_1 = 1 - 1 * (1 * 1) = 0
    B = (sp.kron(sp.identity(W), _t1(W)) + sp.kron(_t1(W), sp.identity(W)) + 0.5 * sp.identity(W * W)).tolil()
    i = 5 * W
    B[i, i] = B[i, i + 1] = B[i + 1, i] = B[i + 1, i + 1] = 1.0
    B = K.as_csr(B.tocsr())
    dB = ops.DeviceCSR.from_scipy(B, DEV)
    assert ops.line_factor_flags(dB, W, "x")[1] == ops.LINE_PIVOT == LR.factor(B, W, "x")[1]
    assert ops.line_factor_flags(dB, W, "y")[1] == 0 == LR.factor(B, W, "y")[1]
    with pytest.raises(ValueError, match=r"level 0.*pivot"):
        Hierarchy(B, hier, DEV).prepare_smoother("Line")


def test_levels_without_the_geometry_are_refused_by_name():
    A1, _ = P.poisson_1d_fd(4096)
    H = Hierarchy(A1, P.geometric_hierarchy_1d(4097, 2), DEV)
    with pytest.raises(ValueError, match=r"level 0.*W == n"):
        H.prepare_smoother("Line")
    # transfers with three entries per direction on the coincident rows (the sparsity of a learned Q): the Galerkin operator
    # of level 1 is a 25-point operator
    A, _ = P.anisotropic_poisson_2d_structured(32, 1e-3, 1.0)
    q = P.pseudo_l2_interpolator_1d(33)
    Q = P.learned_like(sp.kron(q, q, format="csr"), seed=5)
    H = Hierarchy(A, [Q, P.tensor_interpolator_2d(17)], DEV)
    assert H.levels[1].A.nnz > 9 * H.levels[1].n
    with pytest.raises(ValueError, match=r"level 1.*no 3x3 grid geometry"):
        H.prepare_smoother("Line")
    assert H.levels[0].line is not None and "x" in H.levels[0].line      # level 0 itself can run it


def test_entry_points_check_their_arguments():
    """Every bad call answers LMG_ERR_ARG (-1) before anything is launched (the buffers keep their NaNs)."""
    W, Hg = 9, 7
    A = operator("aniso5", W, Hg)
    n = A.shape[0]
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    nan = lambda: torch.full((n,), np.nan, dtype=torch.float64, device=DEV)
    lo, minv, cp, r, x = nan(), nan(), nan(), nan(), nan()
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()
    good_f = [n, W, 0, p(dA.rowptr), p(dA.colidx), p(dA.vals), p(lo), p(minv), p(cp), p(flags), st]
    for at in (3, 4, 5, 6, 7, 8, 9):                                  # NULL pointers
        bad = list(good_f)
        bad[at] = None
        assert L.lmg_line_factor(*bad) == -1, at
    for at, v in ((2, 2), (2, -1), (1, 0), (1, 8), (0, -1)):          # bad dir, bad stride, n % line_stride != 0, n < 0
        bad = list(good_f)
        bad[at] = v
        assert L.lmg_line_factor(*bad) == -1, (at, v)
    good_s = [n, W, 1, 0, 1, p(lo), p(minv), p(cp), p(r), 1.0, p(x), st]
    for at in (5, 6, 7, 8, 10):
        bad = list(good_s)
        bad[at] = None
        assert L.lmg_line_solve(*bad) == -1, at
    for at, v in ((4, 0), (4, -2), (3, -1), (2, 2), (2, -1), (1, 0), (1, 8), (0, -1)):   # step < 1, first < 0, dir, stride
        bad = list(good_s)
        bad[at] = v
        assert L.lmg_line_solve(*bad) == -1, (at, v)
    bad = list(good_s)
    bad[8] = bad[10]                                                   # r aliases x
    assert L.lmg_line_solve(*bad) == -1
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (lo, minv, cp, r, x)) and int(flags.item()) == 0
    with pytest.raises(ValueError):
        ops.line_factor(dA, W, "z")
    with pytest.raises(ValueError):
        ops.line_factor(dA, 8, "x")


# ---- 3. whole solves --------------------------------------------------------------------------------------------------------------
CONFIGS = [("xy", "zebra", 1.0), ("y", "zebra", 1.0), ("xy", "jacobi", 0.8)]


def _problem(name):
    if name == "aniso65_x_weak":
        A, rhs = P.anisotropic_poisson_2d_structured(64, 1e-3, 1.0)
        return A, rhs, P.geometric_hierarchy_2d(65, 4)
    if name == "aniso65_y_weak":
        A, rhs = P.anisotropic_poisson_2d_structured(64, 1.0, 1e-3)
        return A, rhs, P.geometric_hierarchy_2d(65, 4)
    A, rhs = P.variable_coeff_poisson_2d_structured(128, seed=44)
    return A, rhs, P.geometric_hierarchy_2d(129, 4)


def _histories(H, rhs, cycles, cfg, shape="V", graph=False, smoother="Line", steps=1):
    fine = H.levels[0]
    with torch.cuda.stream(H.stream):
        if smoother == "Line":
            H.prepare_smoother("Line", line_dir=cfg[0], line_order=cfg[1])
        fine.b.copy_(dev(rhs.ravel()))
        ops.zero(fine.x)
        g = H.captured_cycle(smoother, steps, cfg[2], "lexicographic", shape=shape) if graph else None
        norms = [H.residual_norm()]
        for _ in range(cycles):
            if g is not None:
                g.launch()
            else:
                H.cycle(smoother, steps, cfg[2], shape=shape)
            norms.append(H.residual_norm())
        x = fine.x.cpu().numpy().copy()
    return np.array(norms), x


def _twin_history(A, rhs, hier, cycles, cfg, shape, H):
    """The twin's history on H's own level operators, the coarsest level solved by H's own direct solver: the twin restates
    the smoother and the cycle, not the Galerkin products and not the direct solver."""
    last = H.levels[-1]

    def coarse(rc):
        with torch.cuda.stream(H.stream):
            last.b.copy_(dev(rc))
            H.coarse_solve()
            return last.x.cpu().numpy().copy()

    ref = LR.LineCycle([l.A.to_scipy() for l in H.levels], [l.P.to_scipy() for l in H.levels[:-1]],
                       [l.R.to_scipy() for l in H.levels[:-1]], coarse, line_dir=cfg[0], line_order=cfg[1], omega=cfg[2])
    return LR.history(ref, A, rhs, cycles, steps=1, shape=shape)


@pytest.fixture(scope="module")
def solved():
    """Per problem: the hierarchy and the eager V(1,1) histories of the three configurations (shared by the tests below)."""
    out = {}
    for name in ("aniso65_x_weak", "aniso65_y_weak", "varcoeff129"):
        A, rhs, hier = _problem(name)
        H = Hierarchy(A, hier, DEV)
        out[name] = (A, rhs, hier, H, {cfg: _histories(H, rhs, 8, cfg) for cfg in CONFIGS})
    return out


@pytest.mark.parametrize("name", ["aniso65_x_weak", "aniso65_y_weak", "varcoeff129"])
def test_solve_histories_match_the_twin_and_graph_replay_matches_eager(solved, name):
    A, rhs, hier, H, eager = solved[name]
    assert [lev.line["W"] for lev in H.levels[:-1]] == ([65, 33, 17] if name != "varcoeff129" else [129, 65, 33])
    for cfg in CONFIGS:
        for shape, cycles in (("V", 8), ("W", 5)):
            got, x = eager[cfg] if shape == "V" else _histories(H, rhs, cycles, cfg, shape)
            want, xw = _twin_history(A, rhs, hier, cycles, cfg, shape, H)
            rel = np.abs(got - want) / want
            print("%s %s %s: history rel. diff max %.3e, reduction %.3e" % (name, cfg, shape, rel.max(), got[-1] / got[0]))
            assert np.all(rel <= 1e-10), (name, cfg, shape, rel)
            gg, xg = _histories(H, rhs, cycles, cfg, shape, graph=True)
            assert np.array_equal(gg, got) and np.array_equal(xg, x), (name, cfg, shape, "graph replay vs eager")


def test_graph_key_carries_the_line_configuration(solved):
    H = solved["aniso65_x_weak"][3]
    with torch.cuda.stream(H.stream):
        g1 = H.captured_cycle("Line", 1, 1.0, "lexicographic", line_dir="xy", line_order="zebra")
        g2 = H.captured_cycle("Line", 1, 1.0, "lexicographic")
        g3 = H.captured_cycle("Line", 1, 1.0, "lexicographic", line_dir="y")
        g4 = H.captured_cycle("Line", 1, 1.0, "lexicographic", line_dir="xy", line_order="zebra")
    assert g1 is g2 and g3 is not g1 and g4 is g1


@pytest.mark.parametrize("weak", ["x", "y"])
def test_convergence_conditions_hold_on_the_device(solved, weak):
    A, rhs, hier, H, eager = solved["aniso65_%s_weak" % weak]
    red = {cfg[:2]: h[-1] / h[0] for cfg, (h, _) in eager.items()}
    for d in "xy":
        if (d, "zebra") not in red:
            h, _ = _histories(H, rhs, 8, (d, "zebra", 1.0))
            red[d, "zebra"] = h[-1] / h[0]
    h, _ = _histories(H, rhs, 8, (None, None, 0.8), smoother="Jacobi")
    red["point", "jacobi"] = h[-1] / h[0]
    print("weak direction %s: %s" % (weak, {k: "%.2e" % v for k, v in sorted(red.items())}))
    strong = "y" if weak == "x" else "x"
    assert red["xy", "zebra"] <= 1e-8
    assert red[strong, "zebra"] <= 1e-8
    assert red["xy", "jacobi"] <= 1e-8
    assert red["point", "jacobi"] >= 1e-2
    assert red[weak, "zebra"] >= 1e-2


def test_solver_front_end(solved):
    from learnmultigrid_amd.solvers import HierarchyMG
    A, rhs, hier, H, eager = solved["aniso65_x_weak"]
    kw = dict(levels=4, smooth_steps=1, max_iterations=10, error=1e-30, smoother="Line", smoother_semantics="as_named")
    tracks = {}
    for graph in (False, True):
        mg = HierarchyMG(A, rhs.copy(), hier)
        mg.solve(use_graph=graph, line_dir="xy", line_order="jacobi", omega=0.8, **kw)
        tracks[graph] = mg.get_track_res().copy()
    assert np.array_equal(tracks[False], tracks[True])
    # track[0] is the reference's ||1||; track[k] the residual after k cycles
    want = eager["xy", "jacobi", 0.8][0]
    np.testing.assert_allclose(tracks[True][1:9, 0], want[1:9], rtol=1e-10, atol=0)
    # as shipped the name is ignored: forward Gauss-Seidel runs
    kw2 = dict(levels=4, smooth_steps=1, max_iterations=3, error=1e-8)
    a = HierarchyMG(A, rhs.copy(), hier)
    a.solve(smoother="Line", line_dir="nonsense", **kw2)
    g = HierarchyMG(A, rhs.copy(), hier)
    g.solve(smoother="GaussSeidel", **kw2)
    assert np.array_equal(a.get_track_res(), g.get_track_res())
    with pytest.raises(ValueError, match="line_dir"):
        HierarchyMG(A, rhs.copy(), hier).solve(line_dir="yx", **kw)
    # one cycle through v_cycle / w_cycle / f_cycle
    mg = HierarchyMG(A, rhs.copy(), hier)
    ref = LR.LineCycle.galerkin(A, hier, line_dir="y", line_order="zebra")
    for fn, shape in ((mg.v_cycle, "V"), (mg.w_cycle, "W"), (mg.f_cycle, "F")):
        u = fn(mg.matrix, np.zeros((A.shape[0], 1)), rhs, "Line", 1, 1e-8, 4, first_call=True, smoother_semantics="as_named",
               line_dir="y")
        w = ref.cycle(np.zeros(A.shape[0]), rhs.ravel(), steps=1, shape=shape)
        np.testing.assert_allclose(u.ravel(), w, rtol=0, atol=1e-10 * np.abs(w).max())


# ---- 4. symmetry and MG-PCG ----------------------------------------------------------------------------------------------------
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


def test_the_line_cycle_is_a_symmetric_operator():
    """M = one cycle from a zero iterate.  Every half-sweep is x += omega B (b - A x) with B symmetric when A is (the inverse of
    a symmetric block-diagonal part); the post-smoothing half runs the half-sweeps of the pre-smoothing half in reverse, its
    adjoint, so with R = P^T, Galerkin coarse operators and the direct coarse solve the cycle is a symmetric operator."""
    A, rhs, hier = _problem("aniso65_x_weak")
    A = symmetric_form(A)
    H = Hierarchy(A, hier, DEV)
    rng = np.random.default_rng(2024)
    n = A.shape[0]
    u, v = rng.random(n), rng.random(n)

    def M(w, steps, omega, shape):
        with torch.cuda.stream(H.stream):
            H.levels[0].b.copy_(dev(w))
            H.cycle("Line", steps, omega, x_is_zero=True, shape=shape)
            return H.levels[0].x.cpu().numpy().copy()

    for cfg, steps, shape in ((("xy", "zebra", 1.0), 1, "V"), (("xy", "zebra", 1.0), 2, "W"), (("xy", "jacobi", 0.8), 1, "V"),
                              (("y", "zebra", 1.0), 1, "V")):
        with torch.cuda.stream(H.stream):
            H.prepare_smoother("Line", line_dir=cfg[0], line_order=cfg[1])
        a, b = float(np.dot(M(u, steps, cfg[2], shape), v)), float(np.dot(u, M(v, steps, cfg[2], shape)))
        print("%s %d %s: <Mu, v> = %.17g, <u, Mv> = %.17g, rel. diff %.3e" % (cfg, steps, shape, a, b, abs(a - b) / abs(a)))
        assert abs(a - b) <= 1e-12 * abs(a)


def test_mg_pcg_with_the_line_cycle():
    from learnmultigrid_amd.solvers import CG
    A, rhs, hier = _problem("aniso65_x_weak")                        # epsilon = 1e-3
    H = Hierarchy(A, hier, DEV)
    its = {}
    for sm, kw in (("Line", dict(precond_omega=1.0)), ("Jacobi", {})):
        cg = CG(A, rhs.copy())
        cg.solve(max_iterations=500, error=1e-8, preconditioner=H, precond_smoother=sm, precond_steps=1, **kw)
        assert cg.get_track_res()[-1, 0] <= 1e-8, sm
        its[sm] = cg.get_iterations()
    print("MG-PCG, 65^2, ax = 1e-3, one smoothing step: Line %d iterations, Jacobi(0.8) %d" % (its["Line"], its["Jacobi"]))
    assert its["Line"] < its["Jacobi"]


# ---- 5. rebuild_numeric -----------------------------------------------------------------------------------------------------------
def test_rebuild_numeric_gives_the_history_of_a_fresh_hierarchy():
    m = 64
    hier = P.geometric_hierarchy_2d(m + 1, 3)
    A0, rhs = P.variable_coeff_poisson_2d_structured(m, seed=44)
    A1, _ = P.variable_coeff_poisson_2d_structured(m, seed=45)
    A0, A1 = K.as_csr(A0), K.as_csr(A1)
    assert np.array_equal(A0.indices, A1.indices)
    cfg = ("xy", "zebra", 1.0)
    H = Hierarchy(A0, hier, DEV)
    _histories(H, rhs, 1, cfg)
    with torch.cuda.stream(H.stream):
        H.rebuild_numeric(dev(A1.data))
    assert H.line_key() == ("xy", "zebra")
    got, x = _histories(H, rhs, 4, cfg)
    want, xw = _histories(Hierarchy(A1, hier, DEV), rhs, 4, cfg)
    assert np.array_equal(got, want) and np.array_equal(x, xw)


# ---- 6. torch.ops -----------------------------------------------------------------------------------------------------------------
def test_torch_ops_equal_the_ctypes_path():
    ops.register_torch_ops()
    Wg, Hg = 40, 35
    A = operator("varcoeff5", Wg, Hg)
    n = A.shape[0]
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    rng = np.random.default_rng(6)
    x0, r0 = rng.standard_normal(n), rng.standard_normal(n)
    for d in "xy":
        fac, flags = ops.line_factor_flags(dA, Wg, d)
        lo, minv, cp, f2 = torch.ops.lmg.line_factor(dA.rowptr, dA.colidx, dA.vals, Wg, d)
        assert f2 == flags == 0
        assert all(torch.equal(a, b) for a, b in zip(fac, (lo, minv, cp)))
        x1, r1, x2, r2 = dev(x0), dev(r0), dev(x0), dev(r0)
        ops.line_solve(Wg, d, 1, 2, fac, r1, 0.8, x1)
        torch.ops.lmg.line_solve(Wg, d, 1, 2, lo, minv, cp, r2, 0.8, x2)
        assert torch.equal(x1, x2) and torch.equal(r1, r2) and not torch.equal(x1, dev(x0))
