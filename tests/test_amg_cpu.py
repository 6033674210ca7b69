"""What can be said about the classical AMG setup (learnmultigrid_amd/amg.py, csrc/amg.hip) without a GPU: the invariants of
the plain-Python twin of its rules (tests/amg_ref.py), the twin's convergence through the oracle's cycle, Hierarchy with a
callable and with DeviceCSR transfers on CPU tensors, and the argument refusals of every lmg_amg_* entry point."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_cases as C
import amg_ref as R
import cpu_ops_shim as shim
from learnmultigrid_amd import _lib, amg, problems as P
from learnmultigrid_amd.hierarchy import Hierarchy
from learnmultigrid_amd.ops import DeviceCSR
from learnmultigrid_amd.solvers import ClassicalAMG, Multigrid

EPS = np.finfo(np.float64).eps
CASES = sorted(C.case_matrices())


def rows(M):
    return [set(int(j) for j in M.indices[M.indptr[i]:M.indptr[i + 1]]) for i in range(M.shape[0])]


def zero_sum_rows(A):
    """Rows whose entries sum to zero (to rounding of the sum itself)."""
    total = np.asarray(A.sum(axis=1)).ravel()
    scale = np.asarray(abs(A).sum(axis=1)).ravel()
    return (scale > 0) & (np.abs(total) <= 4 * EPS * scale)


# ---- invariants of the twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_split_invariants(name):
    """The independence of the C nodes, as the rules give it.  Step (b) makes an undecided i fine only through a flagged j in
    S_i, so a node that a coarse node depends on, and that does not depend on it, stays undecided and may become coarse in a
    later round: with an unsymmetric S two C nodes can be joined by a ONE-WAY edge of S (on jittered_poisson_2d(32) 2 such
    pairs among 328 C nodes, 1 on jittered_poisson_2d(8) with theta = 1, none on the other case matrices).  What holds, and
    is asserted: no two C nodes of one round are joined in S u S^T; no two C nodes are joined both ways -- so where S is
    symmetric no two C nodes are joined at all --; and where C nodes i, j have j in S_i, i was coarse before j.  (No rule
    gives both "no C-C edge in S u S^T" and "every F node has a C node in S_i" for every unsymmetric S: S_0 = {1}, S_1 = {2},
    S_2 = {0} admits one C node, and one of the other two then has no C node in its row.)"""
    A, theta = C.case_matrices()[name]
    S = R.strength(A, theta)
    when = []
    state, rank, n_c, rounds = R.pmis(S, decided=when)
    out = rows(S)
    back = rows(sp.csr_matrix(S.T))
    assert set(np.unique(state)) <= {R.COARSE, R.FINE, R.FINE0}
    # F0 is exactly the set of rows with no strong entry
    assert [i for i in range(A.shape[0]) if state[i] == R.FINE0] == [i for i in range(A.shape[0]) if not out[i]]
    coarse = set(int(i) for i in np.flatnonzero(state == R.COARSE))
    one_way = 0
    for i in coarse:
        for j in (out[i] | back[i]) & coarse - {i}:
            assert when[i] != when[j]
            assert not (j in out[i] and j in back[i])
            if j in out[i]:
                assert when[i] < when[j]
                one_way += 1
    print(name, "C-C one-way edges:", one_way)
    if (S != S.T).nnz == 0:
        assert one_way == 0
    for i in np.flatnonzero(state == R.FINE):
        assert out[i] & coarse                                    # every other F node has a C node in S_i
    assert n_c == len(coarse) and np.array_equal(rank[state == R.COARSE], np.arange(n_c))
    assert (rounds == 0) == (S.nnz == 0)


@pytest.mark.parametrize("split", ["pmis", "greedy"])
@pytest.mark.parametrize("name", CASES)
def test_interpolation_invariants(name, split):
    A, theta = C.case_matrices()[name]
    S = R.strength(A, theta)
    state, rank, n_c, _ = R.split_of(S, split)
    if n_c in (0, A.shape[0]):
        assert R.transfer(A, theta, split)[0] is None
        return
    P0 = R.direct_interpolation(A, S, state, rank)
    before = R.smooth_rows(A, P0, state, rank)
    P1 = R.smooth_interpolation(A, P0, state, rank)
    assert P0.shape == P1.shape == (A.shape[0], n_c)
    zs = zero_sum_rows(A)
    filled = np.diff(P0.indptr) > 0
    for i in range(A.shape[0]):
        r0, r1 = R.row_of(P0, i), R.row_of(P1, i)
        if state[i] == R.COARSE:
            assert r0 == r1 == ([int(rank[i])], [1.0])            # C rows of P are identity
            continue
        if state[i] == R.FINE0:
            assert r0 == r1 == ([], [])
            continue
        assert r0[0] == sorted(r0[0]) and r1[0] == sorted(r1[0])
        # dropped entries are below the threshold, kept entries are at or above it
        kept, thr = R.truncate_row(before[i], 0.2)
        assert [c for c, _ in kept] == r1[0]
        for c, v in before[i]:
            assert (abs(v) >= thr) == (c in r1[0])
        if not zs[i] or not filled[i]:
            continue
        # a zero-row-sum row: its fine row of P sums to 1 within 4 eps (row length) ...
        cols, _ = R.row_of(A, i)
        assert abs(sum(r0[1]) - 1.0) <= 4 * EPS * len(cols)
        # ... and still after the Jacobi step, where every neighbour's row of P sums to 1 itself: the step subtracts
        # (sum_k a_ik rowsum(P_k)) / a_ii, which is the row sum of A only then
        if all(state[k] == R.COARSE or (state[k] == R.FINE and zs[k] and filled[k]) for k in cols):
            assert abs(sum(r1[1]) - 1.0) <= 4 * EPS * max(len(cols), len(before[i]))


def test_refusal_names_the_row():
    A, state, row = C.overflow_row()
    S = R.strength(A)
    with pytest.raises(R.Refused) as e:
        R.direct_interpolation(A, S, state, R.ranks(state)[0])
    assert (e.value.rule, e.value.row) == ("pivot", row)


def test_greedy_is_the_host_rule():
    from learnmultigrid_amd import ops
    _lib.build()
    for name in ("jittered32", "two_blocks", "no_diagonal", "diagonal"):
        A, theta = C.case_matrices()[name]
        S = R.strength(A, theta)
        state = R.greedy(S)[0]
        assert np.array_equal(state == R.COARSE, ops.host_greedy_cf(S) != 0), name


# ---- convergence of the twin through the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.problems()))
def test_twin_converges(name):
    """V(2,2) damped Jacobi (0.8) on the twin's hierarchy (max_coarse=100: three or more levels at 33^2) to 1e-8 ||b||.  With
    the hash of amg_ref.hash32 the twin needs 17 cycles on poisson_2d_structured(32), 20 on jittered_poisson_2d(32), 22 on
    its renumbered copy, 19 on the anisotropic problem and 18 on variable_coeff_poisson_2d_structured(32) (the NumPy prototype
    of the rules, with another hash: 17, 20, 20, 19, 18); without the Jacobi step on P jittered_poisson_2d(32) needs 41 (38)."""
    A, b = C.problems()[name]
    Ps, As, _ = C.twin_hierarchy(name)
    assert len(As) >= 3
    got = C.cycles_needed(C.oracle_history(A, b, Ps))
    print(name, [M.shape[0] for M in As], got)
    assert got is not None and got <= C.CAP


def test_jacobi_step_pays():
    A, b = C.problems()["jittered"]
    with_step = C.cycles_needed(C.oracle_history(A, b, C.twin_hierarchy("jittered")[0]))
    without = C.cycles_needed(C.oracle_history(A, b, C.twin_hierarchy("jittered", interp_sweeps=0)[0], cap=100))
    print(with_step, without)
    assert with_step is not None and (without is None or without > with_step)


def test_anisotropic_geometric_hierarchy_stalls():
    """The contrast the GPU test draws, on the oracle: under V(2,2) damped Jacobi the geometric hierarchy of the anisotropic
    problem (0.01 u_xx + u_yy) has not reached 1e-8 ||b|| after 30 cycles (full coarsening against point smoothing), the
    algebraic one has after 19."""
    A, b = C.problems()["anisotropic"]
    assert C.cycles_needed(C.oracle_history(A, b, P.geometric_hierarchy_2d(33, 3))) is None
    assert C.cycles_needed(C.oracle_history(A, b, C.twin_hierarchy("anisotropic")[0])) is not None


# ---- Hierarchy with a callable and with DeviceCSR transfers -------------------------------------------------------------------
def level_arrays(H):
    out = []
    for lev in H.levels:
        for M in (lev.A, lev.P, lev.R):
            out.append(None if M is None else (M.shape, M.rowptr.numpy().copy(), M.colidx.numpy().copy(), M.vals.numpy().copy()))
    return out


def assert_same_levels(H0, H1):
    a0, a1 = level_arrays(H0), level_arrays(H1)
    assert len(a0) == len(a1)
    for x, y in zip(a0, a1):
        assert (x is None) == (y is None)
        if x is not None:
            assert x[0] == y[0] and all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:]))


def test_hierarchy_takes_device_csr_and_callable():
    A, _ = C.problems()["jittered"]
    Ps = C.twin_hierarchy("jittered")[0]
    H0 = Hierarchy(A, Ps, "cpu", ops_mod=shim)
    dPs = [DeviceCSR.from_scipy(p, "cpu") for p in Ps]
    H1 = Hierarchy(A, dPs, "cpu", ops_mod=shim)
    assert all(lev.P is dp for lev, dp in zip(H1.levels, dPs))             # used as they are
    asked = []

    def transfers(l, Al):
        assert isinstance(Al, DeviceCSR)
        asked.append((l, Al.shape[0]))
        return dPs[l] if l < len(dPs) else None

    H2 = Hierarchy(A, transfers, "cpu", ops_mod=shim)
    assert asked == [(l, lev.n) for l, lev in enumerate(H0.levels)]        # once per level, the last answer None
    mixed = Hierarchy(A, lambda l, Al: (Ps + [None])[l], "cpu", ops_mod=shim)
    for H in (H1, H2, mixed):
        assert_same_levels(H0, H)
    with pytest.raises(ValueError, match="rows"):
        Hierarchy(A, [dPs[1]], "cpu", ops_mod=shim)


def test_callable_that_ends_at_once_is_the_empty_list():
    A, _ = C.problems()["poisson"]
    outcome = []
    for transfers in ([], lambda l, Al: None):
        try:
            H = Hierarchy(A, transfers, "cpu", ops_mod=shim)
            outcome.append(("built", H.sizes))
        except Exception as e:                                              # whichever the code does for an empty list
            outcome.append((type(e), str(e)))
    assert outcome[0] == outcome[1]


def test_classical_amg_keywords():
    """The host-side checks that need no device."""
    with pytest.raises(ValueError, match="split"):
        amg.classical_hierarchy(sp.identity(3, format="csr"), "cpu", split="ruge_stuben")
    with pytest.raises(ValueError, match="theta"):
        amg.strength_device(DeviceCSR.from_scipy(sp.identity(3, format="csr"), "cpu"), theta=1.5)
    assert issubclass(ClassicalAMG, Multigrid)


# ---- argument refusals, without a device ----------------------------------------------------------------------------------
OK, ERR_ARG, ERR_LAUNCH = 0, -1, -3


@pytest.fixture(scope="module")
def L():
    _lib.build()
    lib = _lib.lib()
    if lib.lmg_device_count() > 0:
        pytest.skip("a device is visible: NULL pointers are not handed to entry points that could launch on it")
    return lib


def _arrays():
    i = lambda: np.zeros(8, dtype=np.int32)
    d = lambda: np.ones(8)
    return i, d


def _calls():
    """name -> (arguments as a list, positions of the pointers, positions of (argument, bad value) pairs)."""
    i, d = _arrays()
    keep = []

    def p(a):
        keep.append(a)
        return a.ctypes.data

    n = 3
    smooth = [n, p(i()), p(i()), p(d()), p(i()), p(i()), p(d()), p(i()), p(i()), p(d()), p(i()), p(i()), 1.0, 0.2]
    calls = {
        "lmg_amg_strength_count": ([n, p(i()), p(i()), p(d()), 0.25, p(i()), None], [(4, 1.5), (4, -0.1), (4, float("nan"))]),
        "lmg_amg_strength_fill": ([n, p(i()), p(i()), p(d()), 0.25, p(i()), p(i()), None], [(4, 1.5), (4, float("nan"))]),
        "lmg_amg_pmis_keys": ([n, p(i()), p(i()), p(i()), p(i()), p(i()), None], []),
        "lmg_amg_pmis_select": ([n, p(i()), p(i()), p(i()), p(i()), p(i()), p(i()), p(i()), None], []),
        "lmg_amg_pmis_update": ([n, p(i()), p(i()), p(i()), p(i()), p(i()), p(i()), None], []),
        "lmg_amg_interp_count": ([n, p(i()), p(i()), p(i()), p(i()), None], []),
        "lmg_amg_interp_fill": ([n, p(i()), p(i()), p(d()), p(i()), p(i()), p(i()), p(i()), p(i()), p(i()), p(d()),
                                 p(np.zeros(1, dtype=np.uint64)), None], []),
        "lmg_amg_smooth_count": (smooth + [p(i()), None], [(12, float("inf")), (13, 1.5), (13, -1.0), (13, float("nan"))]),
        "lmg_amg_smooth_fill": (smooth + [p(i()), p(i()), p(d()), None], [(12, float("nan")), (13, 2.0)]),
    }
    return calls, keep


def test_every_entry_point_is_covered():
    from support import header_symbols
    calls, _ = _calls()
    assert sorted(list(calls) + ["lmg_amg_pmis_blocks"]) == sorted(s for s in header_symbols() if s.startswith("lmg_amg_"))


@pytest.mark.parametrize("name", sorted(_calls()[0]))
def test_entry_point_refuses_bad_arguments(L, name):
    calls, keep = _calls()
    args, bad_values = calls[name]
    fn = getattr(L, name)
    pointers = [k for k, a in enumerate(args[:-1]) if isinstance(a, int) and k > 0]
    assert fn(*args) == ERR_LAUNCH                                  # (the checks pass: no device, so the launch fails)
    for k in pointers:
        assert fn(*(args[:k] + [None] + args[k + 1:])) == ERR_ARG, (name, k)
    for size in (-1, 2 ** 31 - 1, 2 ** 31 - 256, 2 ** 40):
        assert fn(*([size] + args[1:])) == ERR_ARG, (name, size)
    for k, v in bad_values:
        assert fn(*(args[:k] + [v] + args[k + 1:])) == ERR_ARG, (name, k, v)
    assert fn(*([0] + args[1:])) == OK                               # nothing to do
    assert fn(*([0, None] + args[2:])) == ERR_ARG                    # ... but still no null pointer
    assert L.lmg_amg_pmis_blocks(0) == 0 and L.lmg_amg_pmis_blocks(-5) == 0
    assert L.lmg_amg_pmis_blocks(256) == 1 and L.lmg_amg_pmis_blocks(257) == 2
