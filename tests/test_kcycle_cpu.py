"""Host logic of the K-cycle on CPU tensors (no GPU): Hierarchy.cycle(shape="K") on the ops shim with the stand-ins of the two
inner steps (kcycle_ref) against the NumPy twin, what a visit launches, who accepts the shape and who refuses it, and what
it buys on a hierarchy that coarsens aggressively."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cpu_ops_shim as shim
import kcycle_ref as KR
from cycle_shapes_ref import ShapeCycle, history
from learnmultigrid_amd import hierarchy as HY
from learnmultigrid_amd import krylov
from learnmultigrid_amd import problems as P
from learnmultigrid_amd.hierarchy import CYCLE_SHAPES, Hierarchy, cycle_children
from learnmultigrid_amd.ops import DeviceCSR


def _geometric(m=64, levels=5):
    A, rhs = P.poisson_2d_structured(m)
    return A, rhs, P.geometric_hierarchy_2d(m + 1, levels)


def _aggregation(side, levels):
    A, rhs = P.poisson_2d_structured(side - 1)
    return A, rhs, KR.aggregation_hierarchy(side, levels)


def _run(H, rhs, cycles, smoother, steps, omega, **kw):
    H.levels[0].b.copy_(torch.from_numpy(rhs.ravel().copy()))
    H.ops.zero(H.levels[0].x)
    norms = []
    for _ in range(cycles):
        norms.append(H.residual_norm())
        H.cycle(smoother, steps, omega, **kw)
    return np.array(norms), H.levels[0].x.numpy().copy()


def _close(got, x, want, xw):
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)
    np.testing.assert_allclose(x, xw, rtol=1e-10, atol=1e-12 * np.abs(xw).max())


# ---- histories ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_inner", KR.K_INNER)
@pytest.mark.parametrize("smoother,omega", [("Jacobi", 0.8), ("GaussSeidel", 1.0)])
def test_geometric_history_matches_the_twin(smoother, omega, k_inner):
    A, rhs, hier = _geometric()
    H = Hierarchy(A, hier, "cpu", ops_mod=KR.ops_namespace())
    got, x = _run(H, rhs, 4, smoother, 2, omega, shape="K", k_inner=k_inner)
    want, xw = history(KR.KCycle(A, hier, k_inner), A, rhs, 4, smoother=smoother, steps=2, omega=omega)
    _close(got, x, want, xw)
    hv, _ = history(ShapeCycle(A, hier, "W"), A, rhs, 4, smoother=smoother, steps=2, omega=omega)
    assert not np.allclose(want[1:], hv[1:], rtol=1e-6, atol=0)              # the K-cycle is told apart from the W-cycle


def test_aggregation_history_matches_the_twin():
    A, rhs, hier = _aggregation(81, 4)
    H = Hierarchy(A, hier, "cpu", ops_mod=KR.ops_namespace())
    assert H.sizes == [81 * 81, 27 * 27, 9 * 9, 3 * 3]
    got, x = _run(H, rhs, 4, "Jacobi", 2, 0.8, shape="K")
    want, xw = history(KR.KCycle(A, hier), A, rhs, 4, smoother="Jacobi", steps=2, omega=0.8)
    _close(got, x, want, xw)


@pytest.mark.parametrize("k_inner", KR.K_INNER)
def test_two_levels_are_a_v_cycle_bit_for_bit(k_inner):
    A, rhs, hier = _geometric(32, 2)
    hk, xk = _run(Hierarchy(A, hier, "cpu", ops_mod=KR.ops_namespace()), rhs, 4, "Jacobi", 2, 0.8, shape="K", k_inner=k_inner)
    hv, xv = _run(Hierarchy(A, hier, "cpu", ops_mod=shim), rhs, 4, "Jacobi", 2, 0.8, shape="V")
    assert np.array_equal(hk, hv) and np.array_equal(xk, xv)


@pytest.mark.parametrize("k_inner", KR.K_INNER)
def test_zero_right_hand_side_gives_exactly_zero(k_inner):
    """rho1 = 0 on every level: the quotients are taken as 0, nothing becomes NaN."""
    A, rhs, hier = _geometric(32, 4)
    H = Hierarchy(A, hier, "cpu", ops_mod=KR.ops_namespace())
    _, x = _run(H, np.zeros_like(rhs), 2, "Jacobi", 2, 0.8, shape="K", k_inner=k_inner)
    assert np.isfinite(x).all() and not x.any()
    for lev in H.levels[1:-1]:
        assert all(np.isfinite(v.numpy()).all() for v in lev.kc)
    assert all(np.isfinite(s.numpy()).all() and s[2] == 0.0 and s[7] == 0.0 for s in H.kscal[1:])


# ---- what a visit launches ------------------------------------------------------------------------------------------------
def _recording_namespace():
    ns = KR.ops_namespace()

    def record(name):
        fn = getattr(ns, name)

        def rec(*args, **kw):
            ns.calls.append((name, tuple(a.data_ptr() if torch.is_tensor(a) else id(a) if isinstance(a, DeviceCSR) else a
                                         for a in args)))
            return fn(*args, **kw)
        setattr(ns, name, rec)

    for name in ("csr_spmv", "kcycle_step1", "kcycle_step2", "dot", "axpby", "copy"):
        record(name)
    return ns


def test_census_of_a_cycle():
    """Per accelerated visit of level l: two products with A_l, one step 1, one step 2, nothing else of the vector ops on
    the level's vectors; 2^(l-1) such visits of level l per cycle, each with two cycle visits of the level, as for W."""
    A, rhs, hier = _geometric(64, 5)
    ns = _recording_namespace()
    H = Hierarchy(A, hier, "cpu", ops_mod=ns)
    H.levels[0].b.copy_(torch.from_numpy(rhs.ravel().copy()))
    H.cycle("Jacobi", 2, 0.8, shape="K")                                    # (the first cycle allocates)
    before = H.memory_bytes()
    ns.calls.clear()
    H.cycle("Jacobi", 2, 0.8, shape="K")
    assert H.memory_bytes() == before
    L = len(H.levels) - 1
    for l in range(1, L):
        lev = H.levels[l]
        own = {t.data_ptr() for t in (lev.x, lev.b, lev.r, lev.tmp) + lev.kc}
        spmv_A = [c for c in ns.calls if c[0] == "csr_spmv" and c[1][0] == id(lev.A)]
        step1 = [c for c in ns.calls if c[0] == "kcycle_step1" and c[1][2] in own]
        step2 = [c for c in ns.calls if c[0] == "kcycle_step2" and c[1][2] in own]
        visits = 2 ** (l - 1)
        assert (len(spmv_A), len(step1), len(step2)) == (2 * visits, visits, visits), l
        assert not [c for c in ns.calls if c[0] in ("dot", "axpby", "copy") and own & set(c[1])], l
        # step 1 writes rt where the second visit reads its right-hand side; x_out is one of the level's own two buffers
        assert all(c[1][4] == lev.kc[0].data_ptr() for c in step1)
        assert all(c[1][7] in (lev.x.data_ptr(), lev.tmp.data_ptr()) for c in step2)
        # the level is entered twice per accelerated visit: its restriction runs 2 * visits times
        assert len([c for c in ns.calls if c[0] == "csr_spmv" and c[1][0] == id(lev.R)]) == 2 * visits
    assert not [c for c in ns.calls if c[0].startswith("kcycle") and c[1][2] in
                {t.data_ptr() for lev in (H.levels[0], H.levels[-1]) for t in (lev.x, lev.b, lev.r, lev.tmp)}]


def test_the_second_visit_leaves_the_first_ones_vectors_alone():
    A, rhs, hier = _geometric(32, 4)
    seen = []

    def step2(k_inner, c1, v1, c2, v2, rt, scal, x_out, partials, form="auto"):
        c1_then, v1_then, b, b_then = step1_saw.pop()
        seen.append((c1.numpy().copy(), v1.numpy().copy(), b.numpy().copy(), c1_then, v1_then, b_then))
        KR.kcycle_step2(k_inner, c1, v1, c2, v2, rt, scal, x_out, partials, form)

    step1_saw = []

    def step1(k_inner, c1, v1, b, rt, scal, partials, form="auto"):
        KR.kcycle_step1(k_inner, c1, v1, b, rt, scal, partials, form)
        step1_saw.append((c1.numpy().copy(), v1.numpy().copy(), b, b.numpy().copy()))

    H = Hierarchy(A, hier, "cpu", ops_mod=KR.ops_namespace(kcycle_step1=step1, kcycle_step2=step2))
    H.levels[0].b.copy_(torch.from_numpy(rhs.ravel().copy()))
    H.cycle("GaussSeidel", 1, 1.0, shape="K")
    assert len(seen) == 1 + 2
    for c1, v1, b, c1_then, v1_then, b_then in seen:               # (as step 2 finds them | as step 1 left them)
        assert np.array_equal(c1, c1_then) and np.array_equal(v1, v1_then) and np.array_equal(b, b_then)
    for lev in H.levels[1:-1]:                       # b is back in its slot for the next restriction
        assert all(lev.b is not w for w in lev.kc) and lev.x is not lev.tmp
        assert all(lev.x is not w and lev.tmp is not w for w in lev.kc)


# ---- names and refusals ---------------------------------------------------------------------------------------------------
def test_names():
    assert CYCLE_SHAPES == ("V", "W", "F")
    assert HY.KRYLOV_SHAPES == ("K",) and HY.K_INNER == KR.K_INNER
    assert cycle_children("K") == ("K", "K")
    for bad in ("k", "KK", None):
        with pytest.raises(ValueError, match="'V', 'W', 'F', 'K'"):
            cycle_children(bad)
    A, rhs, hier = _geometric(16, 3)
    H = Hierarchy(A, hier, "cpu", ops_mod=KR.ops_namespace())
    for bad in ("k", "KK", None):
        with pytest.raises(ValueError):
            H.cycle("Jacobi", 1, 0.8, shape=bad)
    for bad in ("GCR", "cg", None):
        with pytest.raises(ValueError, match="k_inner"):
            H.cycle("Jacobi", 1, 0.8, shape="K", k_inner=bad)


def test_an_ops_module_without_the_two_ops_is_refused_before_any_launch():
    A, rhs, hier = _geometric(16, 3)
    ns = shim.namespace()
    H = Hierarchy(A, hier, "cpu", ops_mod=ns)
    for name in ("csr_jacobi", "vmul", "csr_spmv", "csr_residual_norm2"):            # (the setup is over: a cycle's launches)
        setattr(ns, name, lambda *a, **k: pytest.fail("a launch before the refusal"))
    with pytest.raises(ValueError, match="kcycle_step1 and kcycle_step2"):
        H.cycle("Jacobi", 1, 0.8, shape="K")
    H = Hierarchy(A, hier, "cpu", ops_mod=shim.namespace(kcycle_step1=KR.kcycle_step1))
    with pytest.raises(ValueError, match="lacks kcycle_step2"):
        H.cycle("Jacobi", 1, 0.8, shape="K")


def test_block_cycles_refuse_k_by_name():
    import block_cg_ref as R
    from learnmultigrid_amd.block import BlockCycle
    from learnmultigrid_amd.solvers import GMRES, HierarchyMG
    A, hier, B = R.problem()
    mg = HierarchyMG(A, B[:, :1].copy(), hier, device="cpu")
    with pytest.raises(ValueError, match="Multigrid.solve_many has no 'K' cycle"):
        mg.solve_many(B[:, :2], levels=len(hier) + 1, cycle_shape="K")
    assert mg._hier is None                                                     # nothing was set up
    gm = GMRES(A, B[:, :1].copy(), device="cpu")
    with pytest.raises(ValueError, match="GMRES.solve_many has no 'K' cycle"):
        gm.solve_many(B[:, :2], precond_cycle_shape="K")
    bc = BlockCycle(Hierarchy(A, hier, "cpu", ops_mod=R.block_namespace(shim)), 2)
    with pytest.raises(ValueError, match="BlockCycle has no 'K' cycle"):
        bc.cycle(2, 0.8, "K")
    with pytest.raises(ValueError, match="BlockCycle has no 'K' cycle"):
        bc.apply(bc.levels[0].b, None, 2, 0.8, "K")


def test_cg_and_the_distributed_cycle_refuse_k():
    import block_cg_ref as R
    from learnmultigrid_amd.dist import DistributedVCycle
    from learnmultigrid_amd.solvers import CG
    A, _, B = R.problem()
    cg = CG(A, B[:, :1].copy(), device="cpu")
    with pytest.raises(ValueError, match="'V' or 'W'.*got 'K'"):
        cg.solve(precond_cycle_shape="K")
    with pytest.raises(ValueError, match="'V' or 'W'.*got 'K'"):
        cg.solve_many(B[:, :2], precond_cycle_shape="K")
    with pytest.raises(ValueError, match="the distributed cycle has no 'K' cycle"):
        DistributedVCycle(None, "cpu", ops_mod=shim, cycle_shape="K")           # (before any collective call)
    with pytest.raises(ValueError, match="'V' shape only"):
        DistributedVCycle(None, "cpu", ops_mod=shim, cycle_shape="W")


def test_keywords_of_the_front_ends():
    from learnmultigrid_amd.solvers.GMRES import check_keywords
    ok = dict(restart=10, max_vectors=65, precond_smoother="Jacobi", precond_cycle_shape="K", precond_gs_sweep="forward",
              precond_line_dir="xy", precond_line_order="zebra")
    assert check_keywords(**ok) == (("forward", "forward"), {})
    with pytest.raises(ValueError):
        check_keywords(**dict(ok, precond_cycle_shape="k"))


def test_the_graph_key_holds_k_inner():
    """captured_cycle on a stand-in of CapturedGraph: one graph per k_inner, the buffers back in their slots, and the work
    vectors exist before the capture starts."""
    class Graph:
        def __init__(self):
            assert H.kscal is not None and all(lev.kc is not None for lev in H.levels[1:-1])

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    A, rhs, hier = _geometric(32, 4)
    H = Hierarchy(A, hier, "cpu", ops_mod=KR.ops_namespace(CapturedGraph=Graph))
    before = [(lev.x, lev.tmp, lev.b) for lev in H.levels]
    g = H.captured_cycle("Jacobi", 2, 0.8, "lexicographic", shape="K")
    assert H.captured_cycle("Jacobi", 2, 0.8, "lexicographic", shape="K", k_inner="gcr") is g
    assert H.captured_cycle("Jacobi", 2, 0.8, "lexicographic", shape="K", k_inner="fcg") is not g
    assert sorted(k[5:7] for k in H._graphs) == [("K", "fcg"), ("K", "gcr")]
    assert all(lev.x is x and lev.tmp is t and lev.b is b for lev, (x, t, b) in zip(H.levels, before))
    gv = H.captured_cycle("Jacobi", 2, 0.8, "lexicographic", shape="V")
    assert [k for k, v in H._graphs.items() if v is gv] == [("Jacobi", 2, 0.8, "lexicographic", ("forward", "forward"), "V")]


# ---- convergence ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aggregation_243():
    A, rhs, hier = _aggregation(243, 5)
    return A, rhs, hier, DeviceCSR.from_scipy(sp.csr_matrix(A), "cpu")


def gmres_iterations(ns, H, dA, rhs, shape, k_inner="gcr"):
    """Iterations of GMRES(10) to 1e-8 |b| with one V(2,2)-shaped cycle of H (damped Jacobi, 0.8) as the preconditioner."""
    fine = H.levels[0]

    def apply_M(src, dst):
        ns.copy(src, fine.b)
        H.cycle("Jacobi", 2, 0.8, x_is_zero=True, shape=shape, k_inner=k_inner)
        ns.copy(fine.x, dst)

    b = torch.from_numpy(rhs.ravel().copy())
    x = torch.zeros_like(b)
    tol = 1e-8 * float(np.linalg.norm(rhs))
    track, its = krylov.fgmres(ns, dA, b, x, apply_M, restart=10, max_iterations=200, error=tol)
    assert track[-1] <= tol, (shape, k_inner, track[-1])
    return its


def test_k_cycles_need_fewer_iterations_where_aggregation_is_aggressive(aggregation_243):
    A, rhs, hier, dA = aggregation_243
    ns = KR.ops_namespace()
    H = Hierarchy(A, hier, "cpu", ops_mod=ns)
    assert len(H.levels) == 5
    its = {shape: gmres_iterations(ns, H, dA, rhs, shape) for shape in ("V", "W")}
    for k_inner in KR.K_INNER:
        its_k = gmres_iterations(ns, H, dA, rhs, "K", k_inner)
        print("GMRES(10) iterations on 243^2, 5 levels of 3x3 aggregation: V %d, W %d, K(%s) %d" % (its["V"], its["W"], k_inner, its_k))
        assert its_k < its["W"] < its["V"], (k_inner, its_k, its)
        assert 2 * its_k <= its["V"], (k_inner, its_k, its)
