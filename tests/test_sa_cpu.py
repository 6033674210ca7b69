"""What can be said about the smoothed-aggregation setup (learnmultigrid_amd/aggregation.py, csrc/sa.hip) without a GPU: the
invariants of the plain-Python twin of its rules (tests/sa_ref.py) on every case matrix, the twin's convergence through the
oracle's cycle, the keyword checks that need no device and the argument refusals of every lmg_sa_* entry point."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_cases as C
import sa_cases as SC
import sa_ref as R
from learnmultigrid_amd import _lib, aggregation, amg
from learnmultigrid_amd.ops import DeviceCSR
from learnmultigrid_amd.solvers import ClassicalAMG, Multigrid, SmoothedAggregationAMG

EPS = np.finfo(np.float64).eps
CASES = sorted(SC.case_matrices())


def within(nb, start, edges):
    """The nodes at most `edges` edges from `start`."""
    seen = {start}
    front = {start}
    for _ in range(edges):
        front = {j for i in front for j in nb[i]} - seen
        seen |= front
    return seen


@pytest.mark.parametrize("name", CASES)
def test_aggregation_invariants(name):
    A, theta, _ = SC.case_matrices()[name]
    n = A.shape[0]
    S = R.symmetric_strength(A, theta)
    agg, n_agg, rounds, state, G = R.aggregate(S)
    nb = R.neighbours(G)
    empty = [i for i in range(n) if S.indptr[i + 1] == S.indptr[i]]
    # isolated nodes are exactly the empty rows of S; they have no aggregate and are nobody's neighbour
    assert [i for i in range(n) if state[i] == R.ISOLATED] == empty == [i for i in range(n) if agg[i] < 0]
    assert set(np.unique(state)) <= {R.ROOT, R.COVERED, R.ISOLATED}
    assert not set(empty) & {j for row in nb for j in row} and all(not nb[i] for i in empty)
    # G is symmetric, sorted, without loops, and holds every strong pair of non-isolated nodes
    assert (G != G.T).nnz == 0 and all(row == sorted(set(row)) and i not in row for i, row in enumerate(nb))
    for i in range(n):
        for j in S.indices[S.indptr[i]:S.indptr[i + 1]]:
            assert (j in nb[i]) == (j not in empty)
    # every non-isolated node is in exactly one aggregate, numbered 0 .. n_agg - 1
    assert set(agg[agg >= 0]) == set(range(n_agg))
    roots = [int(i) for i in np.flatnonzero(state == R.ROOT)]
    assert len(roots) == n_agg and [int(agg[r]) for r in roots] == list(range(n_agg))
    # roots are pairwise more than two edges apart; each aggregate holds one root and every member is within two edges of it
    for r in roots:
        near = within(nb, r, 2)
        assert not (near - {r}) & set(roots)
        members = set(int(i) for i in np.flatnonzero(agg == agg[r]))
        assert members & set(roots) == {r} and members <= near
    assert (rounds == 0) == (S.nnz == 0)
    # a non-isolated node without neighbours is an aggregate of its own
    for i in range(n):
        if i not in empty and not nb[i]:
            assert state[i] == R.ROOT and np.count_nonzero(agg == agg[i]) == 1


@pytest.mark.parametrize("name", CASES)
def test_prolongator_invariants(name):
    A, theta, _ = SC.case_matrices()[name]
    B = SC.candidate(name)
    n = A.shape[0]
    P, Bc, info, parts = R.transfer(A, B, theta)
    agg = parts["agg"]
    if info["n_agg"] in (0, n):
        assert P is None and Bc is None
        return
    T = parts["T"]
    live = agg >= 0
    size = max(np.bincount(agg[live]))
    assert T.shape == P.shape == (n, info["n_agg"]) and np.array_equal(np.diff(T.indptr), live.astype(int))
    # the columns of T are orthonormal and T Bc = B on the aggregated rows, to the rounding of the sums (one term per member)
    assert abs(T.T @ T - sp.identity(info["n_agg"])).max() <= 4 * EPS * size
    assert np.all(np.abs(T @ Bc - B)[live] <= 4 * EPS * np.abs(B)[live])
    assert np.all(Bc > 0)
    # rows of P are empty exactly on the isolated nodes, its columns ascend, and it holds T's pattern
    assert np.array_equal(np.diff(P.indptr) > 0, live)
    for i in range(n):
        cols = [int(c) for c in P.indices[P.indptr[i]:P.indptr[i + 1]]]
        assert list(cols) == sorted(set(cols)) and (not live[i] or agg[i] in cols)
    # plain aggregation: omega = 0 leaves the values of T on the pattern of A T
    P0 = R.smooth_prolongator(A, T, agg, 0.0)
    assert np.array_equal(P0.indptr, P.indptr) and np.array_equal(P0.indices, P.indices) and abs(P0 - T).max() == 0.0


def test_a_candidate_that_vanishes_on_an_aggregate_is_refused_with_its_row():
    A, B, row = SC.zero_candidate()
    with pytest.raises(R.Refused) as e:
        R.transfer(A, B)
    assert (e.value.rule, e.value.row) == ("candidate", row)
    bad = B.copy()
    bad[0] = np.inf
    with pytest.raises(R.Refused) as e:
        R.tentative(*R.aggregate(R.symmetric_strength(A))[:2], bad)
    assert (e.value.rule, e.value.row) == ("candidate", 0)


# ---- convergence of the twin through the oracle ---------------------------------------------------------------------------------
# name -> (level sizes, V(2,2) damped Jacobi 0.8 cycles, V(2,2) Gauss-Seidel cycles) to 1e-8 ||b||, max_coarse=100: the twin's
# own counts, measured here through oracle_history; they equal those of the NumPy prototype of the rules.
PINNED = {"poisson": ([1089, 140, 9], 44, 25), "jittered": ([1089, 96], 45, 28), "renumbered": ([1089, 97], 50, 30),
          "variable": ([1089, 140, 9], 46, 26), "anisotropic": ([1089, 268, 78], 31, 21)}


@pytest.mark.parametrize("name", sorted(SC.problems()))
def test_twin_converges_in_the_pinned_number_of_cycles(name):
    A, b = SC.problems()[name]
    Ps, As, _ = SC.twin_hierarchy(name)
    jac = SC.cycles_needed(SC.oracle_history(A, b, Ps, cap=SC.CAP))
    gs = SC.cycles_needed(SC.oracle_history(A, b, Ps, cap=SC.CAP, smoother="GaussSeidel", steps=2))
    print(name, [M.shape[0] for M in As], round(SC.complexity(As), 3), jac, gs)
    assert ([M.shape[0] for M in As], jac, gs) == PINNED[name]


def test_theta_matters_on_the_anisotropic_problem():
    """0.01 u_xx + u_yy: at theta 0 the aggregates ignore the direction of the strong coupling and V(2,2) damped Jacobi has
    not reached 1e-8 ||b|| after 60 cycles (1.7e-3 ||b||); at theta 0.25 it has (31 cycles)."""
    A, b = SC.problems()["anisotropic"]
    h0 = SC.oracle_history(A, b, SC.twin_hierarchy("anisotropic", theta=0.0)[0], cap=SC.CAP)
    h1 = SC.oracle_history(A, b, SC.twin_hierarchy("anisotropic")[0], cap=SC.CAP)
    print(len(h0) - 1, h0[-1] / h0[0], len(h1) - 1, h1[-1] / h1[0])
    assert SC.cycles_needed(h0) is None and len(h0) - 1 == SC.CAP
    assert SC.cycles_needed(h1) is not None and SC.cycles_needed(h1) <= SC.CAP


def test_operator_complexity_is_below_the_classical_one():
    sa = SC.complexity(SC.twin_hierarchy("jittered")[1])
    classical = SC.complexity(C.twin_hierarchy("jittered")[1])
    print(sa, classical)
    assert sa < classical


# ---- keywords, without a device ----------------------------------------------------------------------------------------------
def test_keywords_are_checked_on_the_host():
    I3 = sp.identity(3, format="csr")
    for kw in (dict(theta=-0.1), dict(theta=1.5), dict(omega=float("nan")), dict(omega=float("inf")), dict(max_levels=0)):
        with pytest.raises(ValueError):
            aggregation.sa_hierarchy(I3, "cpu", **kw)
    with pytest.raises(ValueError, match="theta"):
        aggregation.symmetric_strength_device(DeviceCSR.from_scipy(I3, "cpu"), theta=2.0)
    with pytest.raises(ValueError, match="one entry per row"):
        aggregation.candidate_device(np.ones(4), 3, "cpu")
    assert issubclass(SmoothedAggregationAMG, Multigrid) and ClassicalAMG.__init__ is not SmoothedAggregationAMG.__init__
    assert issubclass(amg.Refused, ValueError) and "aggregate" in str(amg.Refused("candidate", 3))
    assert "d_i" in str(amg.Refused("pivot", 3))


# ---- argument refusals, without a device ----------------------------------------------------------------------------------
OK, ERR_ARG, ERR_LAUNCH = 0, -1, -3


@pytest.fixture(scope="module")
def L():
    _lib.build()
    lib = _lib.lib()
    if lib.lmg_device_count() > 0:
        pytest.skip("a device is visible: NULL pointers are not handed to entry points that could launch on it")
    return lib


def _calls():
    """name -> (arguments, (position, bad value) pairs); every integer after the first is a pointer unless named in SIZES."""
    keep = []

    def p(a):
        keep.append(a)
        return a.ctypes.data

    i, d = (lambda: p(np.zeros(8, dtype=np.int32))), (lambda: p(np.ones(8)))
    n = 3
    theta_bad = lambda k: [(k, 1.5), (k, -0.1), (k, float("nan"))]
    calls = {
        "lmg_sa_diagonal": ([n, i(), i(), d(), d(), None], []),
        "lmg_sa_strength_count": ([n, i(), i(), d(), d(), 0.25, i(), None], theta_bad(5)),
        "lmg_sa_strength_fill": ([n, i(), i(), d(), d(), 0.25, i(), i(), None], theta_bad(5)),
        "lmg_sa_graph_count": ([n, i(), i(), i(), i(), i(), None], []),
        "lmg_sa_graph_fill": ([n, i(), i(), i(), i(), i(), i(), None], []),
        "lmg_sa_mis2_init": ([n, i(), i(), i(), None], []),
        "lmg_sa_mis2_t1": ([n, i(), i(), i(), i(), None], []),
        "lmg_sa_mis2_t2": ([n, i(), i(), i(), i(), i(), None], []),
        "lmg_sa_mis2_c1": ([n, i(), i(), i(), i(), i(), None], []),
        "lmg_sa_mis2_update": ([n, i(), i(), i(), i(), i(), i(), i(), None], []),
        "lmg_sa_assign1": ([n, i(), i(), i(), i(), i(), None], []),
        "lmg_sa_assign2": ([n, i(), i(), i(), i(), i(), None], []),
        "lmg_sa_tentative_count": ([n, 2, i(), i(), None], [(1, -1), (1, n + 1)]),
        "lmg_sa_tentative_pattern": ([n, 2, i(), d(), i(), i(), d(), None], [(1, -1), (1, n + 1)]),
        "lmg_sa_norms": ([n, i(), i(), d(), d(), p(np.zeros(1, dtype=np.uint64)), None], []),
        "lmg_sa_tentative_fill": ([n, 2, i(), d(), d(), i(), d(), None], [(1, -1), (1, n + 1)]),
        "lmg_sa_row_states": ([n, i(), i(), None], []),
    }
    return calls, keep


SIZES = {"lmg_sa_tentative_count": 1, "lmg_sa_tentative_pattern": 1, "lmg_sa_tentative_fill": 1}     # the position of n_agg


def test_every_entry_point_is_covered():
    from support import header_symbols
    assert sorted(list(_calls()[0]) + ["lmg_sa_blocks"]) == sorted(s for s in header_symbols() if s.startswith("lmg_sa_"))


@pytest.mark.parametrize("name", sorted(_calls()[0]))
def test_entry_point_refuses_bad_arguments(L, name):
    calls, keep = _calls()
    args, bad_values = calls[name]
    fn = getattr(L, name)
    pointers = [k for k, a in enumerate(args[:-1]) if isinstance(a, int) and k > 0 and k != SIZES.get(name)]
    assert fn(*args) == ERR_LAUNCH                                  # (the checks pass: no device, so the launch fails)
    for k in pointers:
        assert fn(*(args[:k] + [None] + args[k + 1:])) == ERR_ARG, (name, k)
    for size in (-1, 2 ** 31 - 1, 2 ** 31 - 256, 2 ** 40):
        assert fn(*([size] + args[1:])) == ERR_ARG, (name, size)
    for k, v in bad_values:
        assert fn(*(args[:k] + [v] + args[k + 1:])) == ERR_ARG, (name, k, v)
    zero = [0] + args[1:]
    if name in SIZES:
        zero[SIZES[name]] = 0
    assert fn(*zero) == OK                                           # nothing to do
    assert fn(*(zero[:SIZES.get(name, 0) + 1] + [None] + zero[SIZES.get(name, 0) + 2:])) == ERR_ARG   # ... but no null pointer
    assert L.lmg_sa_blocks(0) == 0 and L.lmg_sa_blocks(-5) == 0 and L.lmg_sa_blocks(256) == 1 and L.lmg_sa_blocks(257) == 2


def test_assign2_refuses_to_work_in_place(L):
    calls, keep = _calls()
    args = calls["lmg_sa_assign2"][0]
    assert L.lmg_sa_assign2(*(args[:5] + [args[4]] + args[6:])) == ERR_ARG
