"""What can be said about smoothed aggregation for systems (learnmultigrid_amd/aggregation.py, csrc/nsp.hip) without a GPU:
the invariants of the plain-Python twin of its rules (tests/nsp_ref.py) on every case of tests/nsp_cases.py, the elasticity
generator, the twin's convergence through the oracle's cycle, the keyword checks that need no device and the argument
refusals of every lmg_nsp_* entry point."""
import numpy as np
import pytest
import scipy.sparse as sp

import nsp_cases as NC
import nsp_ref as R
import sa_cases as SC
import sa_ref
from learnmultigrid_amd import _lib, aggregation, amg, problems as P
from learnmultigrid_amd.solvers import SmoothedAggregationAMG

EPS = np.finfo(np.float64).eps
CASES = sorted(NC.cases())


# ---- the twin's invariants ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_prolongator_invariants(name):
    A, bs, X = NC.cases()[name]
    n, k = X.shape
    Pm, Bc, info, parts = R.transfer(A, X, bs=bs)
    agg, rows, T = parts["agg"], parts["rows"], parts["T"]
    n_agg = info["n_agg"]
    live = rows >= 0
    m = int(max(np.bincount(rows[live])))                            # the largest member count, in rows
    # sizes: k coarse unknowns per aggregate; k entries per row of an aggregated node at the columns k agg + c, ascending
    assert T.shape == Pm.shape == (n, k * n_agg) and Bc.shape == (k * n_agg, k)
    assert np.array_equal(np.diff(T.indptr), k * live.astype(int))
    for i in np.flatnonzero(live):
        assert list(T.indices[T.indptr[i]:T.indptr[i + 1]]) == [k * rows[i] + c for c in range(k)]
    # isolated nodes are the empty rows of S(C), and exactly their rows of T and P are empty
    S = parts["S"]
    assert np.array_equal(agg < 0, np.diff(S.indptr) == 0)
    assert np.array_equal(np.diff(Pm.indptr) > 0, live)
    for i in range(n):
        cols = [int(c) for c in Pm.indices[Pm.indptr[i]:Pm.indptr[i + 1]]]
        assert cols == sorted(set(cols))
    # T^T T = I: two rounds of Cholesky-QR leave the rounding of Gram sums of m terms and of k-term triangular solves
    dev_orth = abs(T.T @ T - sp.identity(k * n_agg)).max()
    # T Bc = X on the aggregated rows: the two triangular solves and the product R' R are backward stable, k terms each, so
    # every entry is off by a multiple of eps of its column's norm over the aggregate; the row count enters the Gram sums
    norms = np.zeros((n_agg, k))
    np.add.at(norms, rows[live], X[live] ** 2)
    scale = np.sqrt(norms)[rows[live]]
    dev_rec = np.max(np.abs((T @ Bc - X)[live]) / scale)
    print("%s: |T^T T - I| = %.2e (bound %.2e), |T Bc - X| / column norm = %.2e (bound %.2e), smallest pivot ratio %.2e"
          % (name, dev_orth, 4 * k * EPS * m, dev_rec, 4 * EPS * (m + k * k), min(parts["ratios"])))
    assert dev_orth <= 4 * k * EPS * m
    assert dev_rec <= 4 * EPS * (m + k * k)
    # Bc is upper triangular per aggregate with a positive diagonal
    for j in range(n_agg):
        blk = Bc[k * j:k * j + k]
        assert np.array_equal(np.tril(blk, -1), np.zeros((k, k))) and np.all(np.diag(blk) > 0)
    # plain aggregation: omega = 0 leaves the values of T on the pattern of A T
    P0 = sa_ref.smooth_prolongator(A, T, rows, 0.0)
    assert np.array_equal(P0.indptr, Pm.indptr) and np.array_equal(P0.indices, Pm.indices) and abs(P0 - T).max() == 0.0


def test_case_table_has_the_shapes_it_is_there_for():
    shapes = {}
    for name in CASES:
        A, bs, X = NC.cases()[name]
        _, _, info, parts = R.transfer(A, X, bs=bs)
        agg = parts["agg"]
        shapes[name] = (info["n_agg"], int(min(np.bincount(agg[agg >= 0]))), int(max(np.bincount(agg[agg >= 0]))),
                        int(np.count_nonzero(agg < 0)), min(parts["ratios"]))
    print(shapes)
    assert shapes["chain9_k2"][:4] == (3, 3, 3, 0)
    assert shapes["chain1025_k2"][0] == 281 and 6e-7 < shapes["chain1025_k2"][4] < 7e-7     # a second workgroup of aggregates
    assert shapes["star300_k2"][:3] == (1, 301, 301)
    assert shapes["jit8_k3"][:4] == (7, 5, 10, 32)
    for name in ("elasticity8_rbm", "elasticity8_jittered_rbm", "elasticity8_k4", "elasticity8_k6", "elasticity8_k1"):
        assert shapes[name][:4] == (9, 3, 13, 9), name                  # nodes: the smallest aggregate has 6 rows
    assert min(shapes["elasticity8_k%d" % k][4] for k in (4, 5, 6)) >= 4e-2
    assert NC.cases()["elasticity16_level1"][0].shape == (84, 84) and shapes["elasticity16_level1"][0] == 2


def test_k1_on_block_size_1_is_the_single_candidate_path():
    A, b = SC.problems()["jittered"]
    w = SC.wavy(A.shape[0])
    Ps, As, infos = R.sa_transfers(A, B=w.reshape(-1, 1), **SC.SA_KW)
    Ps0, As0, infos0 = sa_ref.sa_transfers(A, B=w, **SC.SA_KW)
    assert len(Ps) == len(Ps0) and all((a != b_).nnz == 0 for a, b_ in zip(Ps, Ps0))
    assert [dict(d, block_size=1, candidates=1) for d in infos0] == infos


def test_refusals_name_the_smallest_row_of_the_aggregate():
    ref = NC.refusals()
    assert {k: v[3] for k, v in ref.items()} == {"singleton": 1, "equal_columns": 0, "inf": 3}
    # node blocks: the row is block_size times the smallest member node
    A, bs, X = NC.cases()["elasticity8_rbm"]
    agg = R.transfer(A, X, bs=bs)[3]["agg"]
    bad = X.copy()
    node = int(np.flatnonzero(agg == agg.max())[0])
    bad[:, 2] = np.where(np.repeat(agg, 2) == agg.max(), bad[:, 0], bad[:, 2])       # two equal columns on the last aggregate
    with pytest.raises(R.Refused) as e:
        R.transfer(A, bad, bs=bs)
    assert (e.value.rule, e.value.row) == ("candidate", 2 * node)


def test_condensation_is_the_frobenius_norm_of_the_blocks():
    for A, bs in ((NC.elasticity(8)[0], 2), (NC.cases()["elasticity16_level1"][0], 3), (NC.explicit_zero_block(), 2)):
        C = R.condense(A, bs)
        N = A.shape[0] // bs
        fold = sp.csr_matrix((np.ones(A.shape[0]), (np.arange(A.shape[0]) // bs, np.arange(A.shape[0]))), shape=(N, A.shape[0]))
        sq, pat = A.copy(), A.copy()
        sq.data, pat.data = A.data ** 2, np.ones(A.nnz)
        count = (fold @ pat @ fold.T).tocsr()                      # the stored entries per block: explicit zeros count
        count.sort_indices()
        assert np.array_equal(C.indptr, count.indptr) and np.array_equal(C.indices, count.indices)
        want = (fold @ sq @ fold.T).toarray()[np.repeat(np.arange(N), np.diff(C.indptr)), C.indices]
        assert np.all(np.abs(C.data ** 2 - want) <= 2 * bs * bs * EPS * want)
        assert all(list(C.indices[C.indptr[i]:C.indptr[i + 1]]) == sorted(set(C.indices[C.indptr[i]:C.indptr[i + 1]]))
                   for i in range(N))
    C = R.condense(NC.explicit_zero_block(), 2)
    assert C[0, 2] == 0.0 and C.nnz == 6 and list(C.indices[:C.indptr[1]]) == [0, 2]      # the explicit zero counts
    assert R.condense(A, 1) is not None and (R.condense(A, 1) != R.canonical(A)).nnz == 0
    with pytest.raises(ValueError):
        R.condense(sp.identity(5, format="csr"), 2)


# ---- the generator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [None, 42])
def test_elasticity_generator(seed):
    m = 32
    A, rhs, B, p = P.elasticity_2d(m, seed=seed)
    s = m + 1
    n = 2 * s * s
    assert A.shape == (n, n) and rhs.shape == (n, 1) and B.shape == (n, 3) and p.shape == (s * s, 2)
    assert abs(A - A.T).max() <= EPS * abs(A).max()
    clamped = np.repeat(np.arange(s * s) % s == 0, 2)
    assert np.array_equal(np.flatnonzero(p[:, 0] == 0.0), np.flatnonzero(clamped[::2]))
    for i in np.flatnonzero(clamped):
        assert list(A.indices[A.indptr[i]:A.indptr[i + 1]]) == [i] and A.data[A.indptr[i]] == 1.0
    assert np.all(rhs[clamped] == 0.0) and np.all(rhs[::2] == 0.0)
    assert 1.0 - 1.0 / m < -rhs.sum() < 1.0                          # the unit force on the unit square, less the clamped nodes' share
    # rigid-body modes: translations and the rotation (-y, x) are in the kernel of the stiffness of every free row that has
    # no clamped neighbour (the elimination removed that neighbour's column)
    assert np.array_equal(B[:, 0], np.tile([1.0, 0.0], s * s)) and np.array_equal(B[:, 1], np.tile([0.0, 1.0], s * s))
    assert np.array_equal(B[0::2, 2], -p[:, 1]) and np.array_equal(B[1::2, 2], p[:, 0])
    near = np.repeat(np.arange(s * s) % s == 1, 2)                   # the nodes of the mesh column next to the clamped one
    free = ~clamped & ~near
    # 14 entries per row at most, each product within eps of |a_ij| |b_j| <= ||A||_max * 1.5
    dev = np.abs(A @ B)[free].max()
    print("seed %r: |A B| = %.2e on rows without a clamped neighbour, ||A||_max = %.2f" % (seed, dev, abs(A).max()))
    assert free.sum() == 2 * (s * s - 2 * s) and dev <= 32 * EPS * abs(A).max()
    assert np.abs(A @ B)[near & ~clamped].max() > 1e-3
    # positive definite with the clamp
    assert np.linalg.eigvalsh(P.elasticity_2d(4, seed=seed)[0].toarray()).min() > 0


# ---- convergence of the twin through the oracle --------------------------------------------------------------------------------
# CG preconditioned by one V(2,2) damped Jacobi 0.5 cycle of the oracle on the twin's transfers of elasticity_2d(16),
# max_coarse=100, to 1e-8 ||b||: the twin's own counts, measured here; they equal those of the NumPy prototype of the rules.
PINNED_LEVELS = {"rbm": [578, 84], "translations": [578, 56], "ones": [578, 30]}
PINNED_CG = {"rbm": 20, "translations": 31, "ones": 58}


def test_twin_cg_iterations_are_the_pinned_ones_and_in_order():
    levels = {w: [M.shape[0] for M in NC.twin_hierarchy(w)[1]] for w in PINNED_CG}
    counts = {w: NC.cg_iterations(w) for w in PINNED_CG}
    print(levels, counts)
    assert levels == PINNED_LEVELS and counts == PINNED_CG
    assert counts["rbm"] < counts["translations"] < counts["ones"]
    Ps, As, infos = NC.twin_hierarchy("rbm", max_coarse=50)
    assert [M.shape[0] for M in As] == [578, 84, 6]
    assert [(d["n_agg"], d["block_size"], d["candidates"]) for d in infos] == [(28, 2, 3), (2, 3, 3)]


def test_three_candidates_beat_one_on_the_scalar_problem():
    """jittered_poisson_2d(32), stationary V(2,2) damped Jacobi 0.8: 25 cycles with [1, x, y] against the 45 that
    tests/test_sa_cpu.py pins for the vector of ones."""
    A, b = SC.problems()["jittered"]
    Ps, As, infos = NC.scalar_xy_hierarchy()
    cycles = SC.cycles_needed(SC.oracle_history(A, b, Ps, cap=SC.CAP))
    print([M.shape[0] for M in As], cycles)
    assert [M.shape[0] for M in As] == [1089, 288, 21] and cycles == 25 < 45
    assert [(d["block_size"], d["candidates"]) for d in infos] == [(1, 3), (3, 3)]


# ---- keywords, without a device ------------------------------------------------------------------------------------------------
def test_keywords_are_checked_on_the_host():
    I6 = sp.identity(6, format="csr")
    bad = (dict(B=np.ones((6, 7))), dict(block_size=0), dict(block_size=-2), dict(block_size=4), dict(block_size=1.5),
           dict(rank_tol=0.0), dict(rank_tol=-1e-12), dict(rank_tol=float("nan")), dict(rank_tol=float("inf")),
           dict(B=np.ones((5, 2))), dict(B=np.ones((7, 1))), dict(B=np.ones((6, 2, 1))), dict(block_size=2, B=np.ones((3, 2))))
    for kw in bad:
        with pytest.raises(ValueError):
            aggregation.sa_hierarchy(I6, "cpu", **kw)
    with pytest.raises(ValueError, match="one entry per row"):
        aggregation.sa_hierarchy(I6, "cpu", B=np.ones(5))
    with pytest.raises(ValueError, match="one entry per row"):
        aggregation.candidates_device(np.ones(4), 3, 1, "cpu")
    with pytest.raises(ValueError, match="block_size"):
        aggregation.candidates_device(None, 7, 2, "cpu")
    with pytest.raises(ValueError, match="candidates"):
        aggregation.candidates_device(None, 14, 7, "cpu")
    # the shapes B may have, and its defaults
    for B in (np.arange(6.0), np.arange(6.0).reshape(6, 1)):
        X = aggregation.candidates_device(B, 6, 1, "cpu")
        assert X.shape == (6, 1) and X.is_contiguous() and np.array_equal(X.numpy().ravel(), np.arange(6.0))
    X = aggregation.candidates_device(np.arange(12.0).reshape(6, 2)[:, ::-1], 6, 3, "cpu")
    assert X.shape == (6, 2) and X.is_contiguous() and X[0].tolist() == [1.0, 0.0]
    assert np.array_equal(aggregation.candidates_device(None, 6, 1, "cpu").numpy(), np.ones((6, 1)))
    assert np.array_equal(aggregation.candidates_device(None, 6, 3, "cpu").numpy(), R.candidates(None, 6, 3))
    assert np.array_equal(R.candidates(None, 6, 3), np.tile(np.eye(3), (2, 1)))
    # the solver passes the keywords through and keys its setup on them
    a = SmoothedAggregationAMG(I6, np.ones((6, 1)), block_size=2, rank_tol=1e-10, device="cpu")
    b = SmoothedAggregationAMG(I6, np.ones((6, 1)), block_size=3, device="cpu")
    assert a._amg["block_size"] == 2 and a._amg["rank_tol"] == 1e-10 and b._amg["rank_tol"] == 1e-12
    assert a._setup_key() != b._setup_key()
    assert a._setup_key() != SmoothedAggregationAMG(I6, np.ones((6, 1)), block_size=2, device="cpu")._setup_key()
    assert issubclass(amg.Refused, ValueError)


# ---- argument refusals, without a device ------------------------------------------------------------------------------------
OK, ERR_ARG, ERR_LAUNCH = 0, -1, -3


@pytest.fixture(scope="module")
def L():
    _lib.build()
    lib = _lib.lib()
    if lib.lmg_device_count() > 0:
        pytest.skip("a device is visible: NULL pointers are not handed to entry points that could launch on it")
    return lib


def _calls():
    """name -> (arguments, positions of the scalars, (position, bad value) pairs, the arguments of an empty input).  Every
    argument before the stream that is no scalar is a pointer; argument 0 is the size the launch covers."""
    keep = []

    def p(a):
        keep.append(a)
        return a.ctypes.data

    i, d = (lambda: p(np.zeros(64, dtype=np.int32))), (lambda: p(np.ones(64)))
    st = lambda: p(np.zeros(1, dtype=np.uint64))
    nonfinite = [float("nan"), float("inf"), -float("inf"), 0.0, -1e-12]
    k_bad = lambda pos: [(pos, 0), (pos, 7), (pos, -1)]
    bs_bad = lambda pos: [(pos, 0), (pos, -1)]
    calls = {
        # (n_nodes, bs, ...)
        "lmg_nsp_condense_count": ([3, 2, i(), i(), i(), None], [1], bs_bad(1), {0: 0}),
        "lmg_nsp_condense_fill": ([3, 2, i(), i(), d(), i(), i(), d(), None], [1], bs_bad(1), {0: 0}),
        # (n_agg, n_nodes, bs, k, m_rowptr, m_colidx, x, rank_tol, r, status)
        "lmg_nsp_gram_chol": ([2, 3, 2, 3, i(), i(), d(), 1e-12, d(), st(), None], [1, 2, 3, 7],
                              bs_bad(2) + k_bad(3) + [(7, v) for v in nonfinite] + [(1, -1), (1, 1), (1, 2 ** 40)], {0: 0}),
        # (n, n_agg, bs, k, ...)
        "lmg_nsp_apply": ([6, 2, 2, 3, i(), d(), d(), d(), None], [1, 2, 3],
                          bs_bad(2) + k_bad(3) + [(1, -1), (1, 4), (2, 4)], {0: 0, 1: 0}),
        "lmg_nsp_tri_product": ([2, 3, d(), d(), d(), None], [1], k_bad(1), {0: 0}),
        "lmg_nsp_tentative_count": ([6, 2, 2, 3, i(), i(), None], [1, 2, 3],
                                    bs_bad(2) + k_bad(3) + [(1, -1), (1, 4), (2, 4)], {0: 0, 1: 0}),
        "lmg_nsp_tentative_fill": ([6, 2, 2, 3, i(), d(), d(), i(), i(), d(), None], [1, 2, 3],
                                   bs_bad(2) + k_bad(3) + [(1, -1), (1, 4), (2, 4)], {0: 0, 1: 0}),
    }
    return calls, keep


def test_every_entry_point_is_covered():
    from support import header_symbols
    assert sorted(_calls()[0]) == sorted(s for s in header_symbols() if s.startswith("lmg_nsp_"))
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("lmg_nsp_")) == sorted(_calls()[0])


@pytest.mark.parametrize("name", sorted(_calls()[0]))
def test_entry_point_refuses_bad_arguments(L, name):
    calls, keep = _calls()
    args, scalars, bad_values, empty = calls[name]
    fn = getattr(L, name)
    pointers = [k for k in range(1, len(args) - 1) if k not in scalars]
    assert fn(*args) == ERR_LAUNCH                                  # (the checks pass: no device, so the launch fails)
    for k in pointers:
        assert fn(*(args[:k] + [None] + args[k + 1:])) == ERR_ARG, (name, k)
    for size in (-1, 2 ** 31 - 1, 2 ** 31 - 256, 2 ** 40):
        assert fn(*([size] + args[1:])) == ERR_ARG, (name, size)
    for k, v in bad_values:
        assert fn(*(args[:k] + [v] + args[k + 1:])) == ERR_ARG, (name, k, v)
    zero = [empty.get(k, a) for k, a in enumerate(args)]
    assert fn(*zero) == OK                                           # nothing to do
    for k in pointers:
        assert fn(*(zero[:k] + [None] + zero[k + 1:])) == ERR_ARG, (name, k)      # ... but no null pointer


def test_sizes_that_overflow_together_are_refused(L):
    calls, keep = _calls()
    big = 2 ** 30
    # n_nodes * bs and k * n_agg beyond the row limit, each factor within it
    a = calls["lmg_nsp_condense_count"][0]
    assert L.lmg_nsp_condense_count(*([big, 2] + a[2:])) == ERR_ARG
    a = calls["lmg_nsp_tri_product"][0]
    assert L.lmg_nsp_tri_product(*([big, 2] + a[2:])) == ERR_ARG
    a = calls["lmg_nsp_tentative_count"][0]
    assert L.lmg_nsp_tentative_count(*([big, big, 1, 2] + a[4:])) == ERR_ARG
    assert L.lmg_nsp_tentative_count(*([7, 2, 2, 3] + a[4:])) == ERR_ARG       # n is no multiple of bs
    a = calls["lmg_nsp_apply"][0]
    assert L.lmg_nsp_apply(*(a[:5] + [a[7]] + a[6:])) == ERR_ARG               # in place
