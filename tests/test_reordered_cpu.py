"""Cycles on operators that are not numbered line by line on a grid, on the CPU (no GPU needed): the helpers of
tests/reorder.py, the hierarchy's host logic through the ops shim against oracle.vcycle_ref.HoistedVCycle under the tolerance
rule of tests/reorder.py, the equivariance of the reference itself, the Line smoother's refusal, and the Chebyshev cycle.

Every (kind, numbering) pair the device tests (tests/test_reordered_gpu.py) compare with the oracle is held here to a TENTH
of the rule's atol between two CPU implementations, so that a device result that only just passes the rule is already ten
times worse than the shim and the oracle are to each other."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")

import chebyshev_ref as C                                        # noqa: E402
import cpu_ops_shim as shim                                      # noqa: E402
import reorder as RO                                             # noqa: E402
from learnmultigrid_amd import problems as P                     # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy               # noqa: E402
from oracle.vcycle_ref import HoistedVCycle                      # noqa: E402

PAIRS = sorted({(k, nb) for k, nb, _m, _l in RO.CYCLE_CASES + RO.OTHER_CASES})
CASES = sorted({(k, nb, m, 3) for k, nb in PAIRS for m in (32, 64)} | set(RO.CYCLE_CASES + RO.OTHER_CASES))


# ---- the helpers -------------------------------------------------------------------------------------------------------------
def test_morton_order_interleaves_the_bits_of_x_and_y():
    assert RO.morton_order(4).tolist() == [0, 1, 4, 5, 2, 3, 6, 7, 8, 9, 12, 13, 10, 11, 14, 15]
    for side in (1, 2, 5, 17, 33):
        o = RO.morton_order(side)
        assert np.array_equal(np.sort(o), np.arange(side * side))
        x, y = o % side, o // side
        code = sum((((x >> k) & 1) << (2 * k)) | (((y >> k) & 1) << (2 * k + 1)) for k in range(8))
        assert np.all(np.diff(code) > 0)
    assert np.array_equal(RO.random_order(10, 7), np.random.default_rng(7).permutation(10))


@pytest.mark.parametrize("kind", RO.KINDS)
def test_reorder_with_no_orders_is_the_identity(kind):
    A, hier, rhs = RO.problem(kind, 16, 3)
    Ap, Hp, bp = RO.reorder(A, list(hier), rhs, [None] * 3)
    for got, want in zip([Ap] + Hp, [A] + list(hier)):
        assert got.has_canonical_format and got.indices.dtype == np.int32 and got.data.dtype == np.float64
        assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
        assert np.array_equal(got.data, want.data)
    assert np.array_equal(bp, rhs)
    with pytest.raises(ValueError):
        RO.reorder(A, list(hier), rhs, [None] * 2)


@pytest.mark.parametrize("numbering", RO.NUMBERINGS)
@pytest.mark.parametrize("kind", RO.KINDS)
def test_galerkin_operators_commute_with_the_renumbering(kind, numbering):
    """R A P of the reordered hierarchy is the reordered R A P of the grid hierarchy: same pattern, values at 1e-13 (the
    sums of a Galerkin entry run in another order)."""
    A, hier, rhs = RO.problem(kind, 32, 3)
    Ap, Hp, bp, orders = RO.reordered(kind, numbering, 32, 3)
    grid, perm = HoistedVCycle(A, list(hier)), HoistedVCycle(Ap, Hp)
    for l, (G, Q) in enumerate(zip(grid.A, perm.A)):
        want, _, _ = RO.reorder(G, [], np.zeros(G.shape[0]), [orders[l]])
        assert np.array_equal(Q.indptr, want.indptr) and np.array_equal(Q.indices, want.indices), l
        assert np.allclose(Q.data, want.data, rtol=1e-13, atol=1e-13 * np.abs(want.data).max()), l
    assert np.array_equal(bp, rhs if orders[0] is None else rhs[orders[0]])
    x = np.random.default_rng(3).standard_normal(A.shape[0])
    xp = x if orders[0] is None else x[orders[0]]
    assert np.allclose(RO.unpermute(Ap @ xp, orders[0]), A @ x, rtol=1e-13, atol=1e-13 * np.abs(A @ x).max())


def test_the_tolerance_is_the_rounding_bound_of_one_residual():
    A = sp.csr_matrix(np.array([[2.0, -1.0, 0.0], [0.0, 3.0, 0.0], [-1.0, -1.0, 4.0]]))
    x, b = np.array([1.0, -2.0, 0.5]), np.array([0.5, 0.0, -1.0])
    want = (3 + 2) * np.finfo(float).eps * np.linalg.norm(np.array([4.0 + 0.5, 6.0, 1.0 + 2.0 + 2.0 + 1.0]))
    assert RO.tolerances(A, x, b) == pytest.approx(want, rel=1e-15)
    RO.assert_history([1.0 + 0.5e-10], [1.0], [1e-300])
    with pytest.raises(AssertionError):
        RO.assert_history([1.0 + 2e-10], [1.0], [1e-300])
    RO.assert_iterate([1.0, 2.0 + 1e-10], [1.0, 2.0])
    with pytest.raises(AssertionError):
        RO.assert_iterate([1.0 + 3e-10, 2.0], [1.0, 2.0])


# ---- the shim under Hierarchy against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,numbering,m,levels", CASES)
def test_shim_cycles_match_the_oracle_within_a_tenth_of_the_rule(kind, numbering, m, levels):
    """Weighted Jacobi (0.8, 2 sweeps) and forward Gauss-Seidel: the history within the rule, the iterate within its rule,
    and the pair of CPU implementations within atol / 10 on every entry."""
    Ap, Hp, bp, _ = RO.reordered(kind, numbering, m, levels)
    H = Hierarchy(Ap, Hp, "cpu", ops_mod=shim)
    for smoother in RO.SMOOTHERS:
        want, atols, xs = RO.reference(kind, numbering, m, levels, smoother)
        got, x = RO.hierarchy_history(H, bp, RO.CYCLES, smoother, RO.STEPS, RO.OMEGA)
        dev = RO.assert_history(got, want, atols, smoother)
        err = RO.assert_iterate(x, xs[-1], smoother)
        print("%s %s %d^2 %s: reference pair %.4f atol, iterate %.2e max|x|, history %.3e -> %.3e"
              % (kind, numbering, m + 1, smoother, dev, err, want[0], want[-1]))
        assert dev <= 0.1, (smoother, dev)
        assert want[-1] < 1e-3 * want[0]                                  # (six cycles that contract: no floor compared)


@pytest.mark.parametrize("numbering", ["morton", "random"])
@pytest.mark.parametrize("kind", ["const", "var"])
def test_the_reference_is_equivariant_under_renumbering(kind, numbering):
    """Jacobi does not know the numbering: the reordered run, un-permuted, is the grid-order run within the rule (the
    Galerkin sums and the coarse LU run in another order).  What licenses the same test on the device."""
    A, hier, rhs = RO.problem(kind, 64, 3)
    _, _, _, orders = RO.reordered(kind, numbering, 64, 3)
    want, atols, xs = RO.oracle_history(HoistedVCycle(A, list(hier)), A, rhs, 4, smoother="Jacobi", steps=RO.STEPS, omega=RO.OMEGA)
    got, _, xp = RO.reference(kind, numbering, 64, 3, "Jacobi")
    dev = RO.assert_history(got[:5], want, atols)
    err = RO.assert_iterate(RO.unpermute(xp[4], orders[0]), xs[4])
    print("%s %s: %.4f atol, iterate %.2e max|x|" % (kind, numbering, dev, err))


# ---- Line: the refusal -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numbering,level", [("morton", 0), ("random", 0), ("mixed", 1)])
def test_line_is_refused_with_the_level_named_and_the_hierarchy_stays_usable(numbering, level):
    """33^2: below twins.DiaTwin.MIN_ROWS every level's offsets are read on the host, so level 0 of "mixed" is found to be a
    grid and level 1 is the one named."""
    Ap, Hp, bp, _ = RO.reordered("var", numbering, 32, 3)
    H = Hierarchy(Ap, Hp, "cpu", ops_mod=shim)
    with pytest.raises(ValueError, match=r"cannot run on level %d \(\d+ rows\): no 3x3 grid geometry" % level):
        H.prepare_smoother("Line")
    with pytest.raises(ValueError, match="level %d " % level):
        H.cycle("Line", 1, 1.0)
    want, atols, xs = RO.reference("var", numbering, 32, 3, "Jacobi")
    got, x = RO.hierarchy_history(H, bp, RO.CYCLES, "Jacobi", RO.STEPS, RO.OMEGA)
    assert RO.assert_history(got, want, atols) <= 0.1
    RO.assert_iterate(x, xs[-1])


# ---- Chebyshev ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,numbering", [("const", "morton"), ("var", "random"), ("learned", "random"), ("var", "mixed")])
def test_chebyshev_cycles_run_and_contract(kind, numbering):
    """The two-launch Chebyshev step (residual, cheby_update) with explicit bounds -- each level's Gershgorin bound from
    tests/chebyshev_ref.py, ratio 4 -- against chebyshev_ref.ChebyCycle, and every cycle contracts."""
    Ap, Hp, bp, _ = RO.reordered(kind, numbering, 32, 3)
    probe = C.ChebyCycle.galerkin(Ap, Hp)
    lmax = [float(v) for v in probe.lmax]
    ref = C.ChebyCycle.galerkin(Ap, Hp, lmax=lmax, ratio=4.0)
    want, atols, xs = RO.oracle_history(ref, Ap, bp, 4, degree=2)
    H = Hierarchy(Ap, Hp, "cpu", ops_mod=shim)
    got, x = RO.hierarchy_history(H, bp, 4, "Chebyshev", 2, cheby_lmax=lmax, cheby_ratio=4.0)
    assert H.cheby_key() == (tuple(lmax), 4.0)
    dev = RO.assert_history(got, want, atols)
    RO.assert_iterate(x, xs[-1])
    print("%s %s: %.4f atol, history %s" % (kind, numbering, dev, got))
    assert np.all(got[2:] < 0.5 * got[1:-1]), got
