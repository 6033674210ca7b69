"""The line relaxation smoother without a GPU: the CPU twin (tests/line_ref.py) against scipy.linalg.solve_banded, the
convergence it is there for (anisotropic operators, where point smoothers stall), Hierarchy.cycle("Line", ...) on the ops shim
against the twin's cycles bit for bit and launch by launch, and the keyword checks of the solver classes."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.linalg import solve_banded

import cpu_ops_shim
import line_ref as LR
from cycle_shapes_ref import ShapeCycle
from learnmultigrid_amd import problems as P
from learnmultigrid_amd.hierarchy import Hierarchy, line_config, line_half_steps
from oracle import kernels as K
from support import galerkin9, to_numpy as _np, to_scipy as _sp

U = 2.0 ** -53


# ---- the twin's tridiagonal solves -----------------------------------------------------------------------------------------
DOMINANT = {
    "aniso_x_weak": lambda: (K.as_csr(P.anisotropic_poisson_2d_structured(32, 1e-3, 1.0)[0]), 33),
    "aniso_y_weak": lambda: (K.as_csr(P.anisotropic_poisson_2d_structured(32, 1.0, 1e-3)[0]), 33),
    "varcoeff": lambda: (K.as_csr(P.variable_coeff_poisson_2d_structured(24)[0]), 25),
    "galerkin9": lambda: (galerkin9(33), 33),
}


@pytest.mark.parametrize("name", sorted(DOMINANT))
@pytest.mark.parametrize("direction", ["x", "y"])
def test_twin_solves_agree_with_solve_banded(name, direction):
    """Componentwise backward error of the twin's T^-1 r in extended precision, max_i |T e - r|_i / (|T| |e| + |r|)_i, at
    most 16 u: the Thomas algorithm is LU without pivoting, whose computed factors of a diagonally dominant tridiagonal
    matrix satisfy |L||U| <= 3 |T|, which bounds the componentwise backward error of the solve by about 12 u (Higham,
    Accuracy and Stability, Thms 9.12 and 9.14; the stored reciprocal pivots add one rounding per element).  Against
    solve_banded the difference then is at most cond_inf(T) times the two backward errors."""
    A, W = DOMINANT[name]()
    n = A.shape[0]
    lo, a, up, flags = LR.tridiagonals(A, W, direction)
    assert flags == 0
    assert np.all(np.abs(a) >= np.abs(lo) + np.abs(up)), "the bound is for diagonally dominant systems"
    fac, flags = LR.factor(A, W, direction)
    assert flags == 0
    r = np.random.default_rng(11).standard_normal(n)
    e, _ = LR.solve(fac, W, direction, 0, 1, r, 1.0, np.zeros(n))          # 0 + 1.0 * e: T^-1 r itself
    worst = worst_fwd = 0.0
    Ls, As, Us, Rs, Es = (LR.by_system(v, W, direction) for v in (lo, a, up, r, e))
    for k in range(As.shape[0]):
        l, d, u, rr, ee = (v[k].astype(np.longdouble) for v in (Ls, As, Us, Rs, Es))
        Te = d * ee
        Te[1:] += l[1:] * ee[:-1]
        Te[:-1] += u[:-1] * ee[1:]
        mag = np.abs(d) * np.abs(ee) + np.abs(rr)
        mag[1:] += np.abs(l[1:] * ee[:-1])
        mag[:-1] += np.abs(u[:-1] * ee[1:])
        worst = max(worst, float(np.max(np.abs(Te - rr) / mag)))
        ab = np.zeros((3, d.size))
        ab[0, 1:], ab[1], ab[2, :-1] = Us[k][:-1], As[k], Ls[k][1:]
        ref = solve_banded((1, 1), ab, Rs[k])
        T = np.diag(As[k]) + np.diag(Ls[k][1:], -1) + np.diag(Us[k][:-1], 1)
        bound = 2 * 16 * U * np.linalg.cond(T, np.inf) * np.abs(ref).max()
        assert np.abs(Es[k] - ref).max() <= bound, (name, direction, k)
        worst_fwd = max(worst_fwd, float(np.abs(Es[k] - ref).max() / np.abs(ref).max()))
    print("%s %s: backward error %.2f u, largest difference to solve_banded %.2e relative" % (name, direction, worst / U, worst_fwd))
    assert worst <= 16 * U


def test_flags_of_the_twin():
    W = 9
    n = W * 7
    helix = sp.diags([-1.0, -1.0, 4.5, -1.0, -1.0], [-W, -1, 0, 1, W], shape=(n, n)).tocsr()      # row i couples to i + 1 always
    assert LR.tridiagonals(helix, W, "x")[3] == LR.COUPLED and LR.tridiagonals(helix, W, "y")[3] == 0
    A = K.as_csr(P.poisson_2d_structured(8)[0]).copy()
    A.data[A.indptr[4]] = 0.0                 # an identity row with a stored 0: element 4 of x-line 0, element 0 of y-line 4
    assert A[4].nnz == 1 and A[4, 4] == 0.0
    for d in "xy":
        assert LR.factor(A, 9, d)[1] == LR.PIVOT


# ---- convergence: what the smoother is for ------------------------------------------------------------------------------------
def _reduction(A, rhs, step, cycles=8):
    A = K.as_csr(A)
    b = rhs.ravel()
    x = np.zeros(A.shape[0])
    r0 = np.sqrt(K.residual(A, x, b)[1])
    for _ in range(cycles):
        x = step(x, b)
    return np.sqrt(K.residual(A, x, b)[1]) / r0


@pytest.fixture(scope="module")
def reductions():
    """||r_8|| / ||r_0|| of V(1,1) on the 65^2 anisotropic problem, 4 levels, per orientation and smoother (computed once)."""
    hier = P.geometric_hierarchy_2d(65, 4)
    out = {}
    for weak, (ax, ay) in (("x", (1e-3, 1.0)), ("y", (1.0, 1e-3))):
        A, rhs = P.anisotropic_poisson_2d_structured(64, ax, ay)
        for cfg in (("xy", "zebra", 1.0), ("x", "zebra", 1.0), ("y", "zebra", 1.0), ("xy", "jacobi", 0.8)):
            ref = LR.LineCycle.galerkin(A, hier, line_dir=cfg[0], line_order=cfg[1], omega=cfg[2])
            out[(weak,) + cfg[:2]] = _reduction(A, rhs, lambda x, b: ref.cycle(x, b, steps=1))
        jac = ShapeCycle(A, hier, "V")
        out[weak, "point", "jacobi"] = _reduction(A, rhs, lambda x, b: jac.cycle(x, b, smoother="Jacobi", steps=1, omega=0.8))
    for k, v in sorted(out.items()):
        print("weak direction %s, %s %s: ||r8|| / ||r0|| = %.2e" % (k + (v,)))
    return out


@pytest.mark.parametrize("weak", ["x", "y"])
def test_line_relaxation_converges_where_point_jacobi_stalls(reductions, weak):
    strong = "y" if weak == "x" else "x"          # the lines to solve run along the strongly coupled direction
    assert reductions[weak, "xy", "zebra"] <= 1e-8
    assert reductions[weak, strong, "zebra"] <= 1e-8
    assert reductions[weak, "xy", "jacobi"] <= 1e-8
    assert reductions[weak, "point", "jacobi"] >= 1e-2
    assert reductions[weak, weak, "zebra"] >= 1e-2


# ---- Hierarchy logic on the shim ------------------------------------------------------------------------------------------------
def _problem(m=32, levels=3, ax=1e-2, ay=1.0):
    A, rhs = P.anisotropic_poisson_2d_structured(m, ax, ay)
    return A, rhs, P.geometric_hierarchy_2d(m + 1, levels)


def _twin_of(H, **kw):
    """The twin on H's own level operators and its coarsest-level solver."""
    last = H.levels[-1]

    def coarse(rc):
        last.b.copy_(torch.from_numpy(rc.copy()))
        H.coarse_solve()
        return last.x.numpy().copy()

    return LR.LineCycle([_sp(l.A) for l in H.levels], [_sp(l.P) for l in H.levels[:-1]], [_sp(l.R) for l in H.levels[:-1]],
                        coarse, **kw)


def _run(H, rhs, cycles, steps, shape, omega, **kw):
    H.levels[0].b.copy_(torch.from_numpy(rhs.ravel().copy()))
    H.ops.zero(H.levels[0].x)
    norms = []
    for _ in range(cycles):
        norms.append(H.residual_norm())
        H.cycle("Line", steps, omega, shape=shape, **kw)
    norms.append(H.residual_norm())
    return np.array(norms), H.levels[0].x.numpy().copy()


@pytest.mark.parametrize("shape", ["V", "W", "F"])
@pytest.mark.parametrize("line_dir,line_order,omega,steps", [("xy", "zebra", 1.0, 1), ("y", "zebra", 1.0, 2), ("x", "jacobi", 0.8, 1),
                                                             ("xy", "jacobi", 0.8, 2)])
def test_hierarchy_cycle_equals_the_twin(shape, line_dir, line_order, omega, steps):
    A, rhs, hier = _problem()
    H = Hierarchy(A, hier, "cpu", ops_mod=cpu_ops_shim.recording_line())
    got, x = _run(H, rhs, 3, steps, shape, omega, line_dir=line_dir, line_order=line_order)
    assert H.line_key() == (line_dir, line_order)
    assert [lev.line["W"] for lev in H.levels[:-1]] == [33, 17]            # from the offsets, on the host
    twin = _twin_of(H, line_dir=line_dir, line_order=line_order, omega=omega)
    want, xw = LR.history(twin, _sp(H.levels[0].A), rhs, 3, steps=steps, shape=shape)
    assert np.array_equal(x, xw)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)


def test_launch_sequence_and_the_reversed_post_smoothing_half():
    A, rhs, hier = _problem(16, 2)
    shim = cpu_ops_shim.recording_line()
    H = Hierarchy(A, hier, "cpu", ops_mod=shim)
    H.prepare_smoother("Line")                                               # the defaults: "xy", "zebra"
    n = A.shape[0]
    assert [c for c in shim.calls if c[0] == "factor"] == [("factor", n, 17, "x"), ("factor", n, 17, "y")]
    H.levels[0].b.copy_(torch.from_numpy(rhs.ravel().copy()))
    del shim.calls[:]
    H.cycle("Line", 1, 1.0, x_is_zero=True)
    fine = [c for c in shim.calls if c[0] in ("solve", "copy") or (c[0] == "residual" and c[1] == n)]
    res, s = ("residual", n), lambda d, f: ("solve", n, d, f, 2, 1.0)
    assert fine == [("copy", n), s("x", 0), res, s("x", 1), res, s("y", 0), res, s("y", 1),
                    res,                                                     # the residual that is restricted
                    res, s("y", 1), res, s("y", 0), res, s("x", 1), res, s("x", 0)]
    assert not [c for c in shim.calls if c[0] == "factor"]                   # nothing is factored inside a cycle
    # all systems from one residual, one direction, damping; two steps
    H.prepare_smoother("Line", line_dir="y", line_order="jacobi")
    del shim.calls[:]
    H.cycle("Line", 2, 0.8)
    fine = [c for c in shim.calls if c[0] == "solve" or (c[0] == "residual" and c[1] == n)]
    sj = ("solve", n, "y", 0, 1, 0.8)
    assert fine == [res, sj, res, sj, res, res, sj, res, sj]
    assert line_half_steps("xy", "zebra") == [("x", 0, 2), ("x", 1, 2), ("y", 0, 2), ("y", 1, 2)]
    assert line_half_steps("xy", "zebra", reverse=True) == [("y", 1, 2), ("y", 0, 2), ("x", 1, 2), ("x", 0, 2)]
    assert line_half_steps("x", "jacobi", reverse=True) == [("x", 0, 1)]


def test_zero_steps_and_unprepared_use():
    A, rhs, hier = _problem(16, 2)
    H = Hierarchy(A, hier, "cpu", ops_mod=cpu_ops_shim.recording_line())
    with pytest.raises(RuntimeError):
        H.smooth(0, "Line", 1, 1.0, "lexicographic")
    H.prepare_smoother("Line", line_dir="x")
    assert set(H.levels[0].line) == {"W", "x"}
    with pytest.raises(ValueError):
        H.smooth(0, "Line", 1, 1.0, "lexicographic", direction="symmetric")


def test_levels_that_cannot_run_it_are_named():
    A1, _ = P.poisson_1d_fd(64)
    H = Hierarchy(A1, P.geometric_hierarchy_1d(65, 2), "cpu", ops_mod=cpu_ops_shim.recording_line())
    with pytest.raises(ValueError, match=r"level 0.*W == n"):
        H.prepare_smoother("Line")
    # a 25-point operator (the square of the 9-point pattern): no 3x3 geometry
    A, rhs, hier = _problem(16, 2)
    G = K.as_csr(sp.csr_matrix(A @ A))
    H = Hierarchy(G, hier, "cpu", ops_mod=cpu_ops_shim.recording_line())
    with pytest.raises(ValueError, match=r"level 0.*no 3x3 grid geometry"):
        H.prepare_smoother("Line")
    # row i coupled to row i + 1 everywhere: an entry across every line end
    W = 17
    helix = sp.diags([-1.0, -1.0, 4.5, -1.0, -1.0], [-W, -1, 0, 1, W], shape=(W * W, W * W)).tocsr()
    for bad in ("x", "xy"):
        H = Hierarchy(helix, hier, "cpu", ops_mod=cpu_ops_shim.recording_line())
        with pytest.raises(ValueError, match=r"level 0.*couples two x-lines"):
            H.prepare_smoother("Line", line_dir=bad)
    H = Hierarchy(helix, hier, "cpu", ops_mod=cpu_ops_shim.recording_line())
    H.prepare_smoother("Line", line_dir="y")
    H.cycle("Line", 1, 1.0)
    # a zero on the diagonal
    Z = K.as_csr(A).copy()
    Z.data[Z.indptr[4]] = 0.0                                                 # (an identity row: nothing else in its pivot)
    H = Hierarchy(Z, hier, "cpu", ops_mod=cpu_ops_shim.recording_line())
    with pytest.raises(ValueError, match=r"level 0.*pivot"):
        H.prepare_smoother("Line")


def test_rebuild_numeric_refreshes_the_factors():
    A, rhs, hier = _problem(16, 3)
    base = K.as_csr(A)
    rng = np.random.default_rng(3)

    def perturbed():
        v = base.data.copy()
        off = v < 0
        v[off] *= 1.0 + 0.3 * rng.random(int(off.sum()))
        return v

    v0, v1 = perturbed(), perturbed()
    mk = lambda v: sp.csr_matrix((v, base.indices.copy(), base.indptr.copy()), shape=base.shape)
    H = Hierarchy(mk(v0), hier, "cpu", ops_mod=cpu_ops_shim.recording_line())
    _run(H, rhs, 1, 1, "V", 1.0, line_dir="xy", line_order="zebra")
    H.rebuild_numeric(torch.from_numpy(v1))
    assert H.line_key() == ("xy", "zebra")
    got, x = _run(H, rhs, 2, 1, "V", 1.0)
    fresh = Hierarchy(mk(v1), hier, "cpu", ops_mod=cpu_ops_shim.recording_line())
    want, xw = _run(fresh, rhs, 2, 1, "V", 1.0)
    assert np.array_equal(got, want) and np.array_equal(x, xw)
    for a, b in zip(H.levels[:-1], fresh.levels[:-1]):
        for d in "xy":
            assert all(np.array_equal(_np(p), _np(q)) for p, q in zip(a.line[d], b.line[d]))


# ---- keywords ------------------------------------------------------------------------------------------------------------------
def test_line_config():
    assert line_config() == ("xy", "zebra") and line_config("y", "jacobi") == ("y", "jacobi")
    for bad in ("yx", "z", "", 3):
        with pytest.raises(ValueError, match="line_dir"):
            line_config(bad, "zebra")
    for bad in ("Zebra", "gs", 1):
        with pytest.raises(ValueError, match="line_order"):
            line_config("x", bad)


def test_solver_keywords():
    from learnmultigrid_amd.smoothing import smoother_options
    from learnmultigrid_amd.solvers.Multigrid import Multigrid
    eff = Multigrid._effective_smoother
    assert eff("Line", "as_shipped") == "GaussSeidel"             # as shipped, the name is ignored: Gauss-Seidel runs
    assert eff("Line", "as_named") == "Line"
    with pytest.raises(ValueError):
        smoother_options("Line", 1, line_dir="yx", line_order="zebra")
    with pytest.raises(ValueError):
        smoother_options("Line", 1, line_dir="xy", line_order="red-black")
    assert smoother_options("Line", 1, line_dir="x", line_order="jacobi") == {"line_dir": "x", "line_order": "jacobi", "line_band": 1}
    # what the solver classes mean by a keyword left out: ("xy", "zebra"), band 1; Chebyshev keeps what the hierarchy has
    assert smoother_options("Line", 1) == {"line_dir": "xy", "line_order": "zebra", "line_band": 1}
    assert smoother_options("Chebyshev", 1) == {"cheby_lmax": None, "cheby_ratio": None}
    # not the Line smoother: the keywords are not looked at
    assert smoother_options("GaussSeidel", 1, line_dir="nonsense", line_order="nonsense") == {}
    for name in ("solve", "v_cycle", "w_cycle", "f_cycle"):
        sig = inspect.signature(getattr(Multigrid, name))
        assert sig.parameters["line_dir"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["line_dir"].default == "xy"
        assert sig.parameters["line_order"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["line_order"].default == "zebra"


def test_solve_rejects_bad_keywords_before_any_gpu_work():
    from learnmultigrid_amd.solvers import CG, GeometricMG
    mg = GeometricMG.__new__(GeometricMG)
    with pytest.raises(ValueError, match="line_dir"):
        GeometricMG.solve.__wrapped__(mg, levels=2, smoother="Line", smoother_semantics="as_named", line_dir="diagonal")
    with pytest.raises(ValueError, match="line_order"):
        GeometricMG.solve.__wrapped__(mg, levels=2, smoother="Line", smoother_semantics="as_named", line_order="lexicographic")
    with pytest.raises(ValueError, match="line_dir"):
        GeometricMG.v_cycle.__wrapped__(mg, None, None, None, "Line", 1, 1e-8, 2, smoother_semantics="as_named", line_dir="z")
    cg = CG.__new__(CG)
    with pytest.raises(ValueError, match="line_order"):
        CG.solve.__wrapped__(cg, precond_smoother="Line", precond_line_order="rb")
    sig = inspect.signature(CG.solve)
    assert sig.parameters["precond_line_dir"].default == "xy" and sig.parameters["precond_line_order"].default == "zebra"


def test_distributed_cycle_rejects_line():
    from learnmultigrid_amd.dist import DistributedVCycle
    D = DistributedVCycle.__new__(DistributedVCycle)
    with pytest.raises(ValueError, match="Line"):
        D.cycle("Line", 1)
    with pytest.raises(ValueError, match="Line"):
        D.make_step("Line", 1, 1.0)


def test_anisotropic_problem():
    A, rhs = P.anisotropic_poisson_2d_structured(8, 0.25, 2.0)
    A0, _ = P.poisson_2d_structured(8)
    assert np.array_equal(A.indptr, A0.indptr) and np.array_equal(A.indices, A0.indices)
    k = 4 * 9 + 4
    assert list(A[k].data) == [-2.0, -0.25, 4.5, -0.25, -2.0] and list(A[k].indices) == [k - 9, k - 1, k, k + 1, k + 9]
    assert A[0].nnz == 1 and A[0, 0] == 1.0 and rhs[0, 0] == 0.0 and rhs[k, 0] == 1.0 / 64
    B, _ = P.anisotropic_poisson_2d_structured(8, 1.0, 1.0)
    assert np.array_equal(B.data, A0.data)
