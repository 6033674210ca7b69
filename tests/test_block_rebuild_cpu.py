"""A BlockCycle across Hierarchy.rebuild_numeric() without a GPU: a BlockCycle built before the rebuild must give, method by
method, the bits of one built after it.  The NumPy block namespace of tests/block_cg_ref.py with two changes that make
staleness show on the host: block_twin hands out a SNAPSHOT of the matrix values (what a sliced-ELL twin of the cycle's own
is on the device), which the stand-in sweeps read and update_values(A) rewrites; and CapturedGraph is an eager stand-in that
counts how often it was created.  The premise test recomputes the figures the device tests (tests/test_block_rebuild_gpu.py)
rest on."""
import numpy as np
import pytest
import torch

import block_cg_ref as C
import block_gmres_ref as G
import block_rebuild_ref as R
import cpu_ops_shim as shim
from learnmultigrid_amd.block import BlockCycle
from krylov_ref import fgmres_ref
from learnmultigrid_amd.hierarchy import Hierarchy
from oracle.vcycle_ref import HoistedVCycle
from support import to_numpy as _np

CYCLES = 4                                                           # (bitwise comparisons: the number of cycles adds nothing)


class Snapshot:
    """Stands for a sliced-ELL twin that is not the matrix's own: the pattern of A and a COPY of its values."""

    def __init__(self, A):
        self.shape, self.n, self.rowptr, self.colidx = A.shape, A.shape[0], A.rowptr, A.colidx
        self.vals = A.vals.clone()
        self.updates = 0

    def update_values(self, A):
        assert A.shape == self.shape and A.vals.numel() == self.vals.numel()
        self.vals.copy_(A.vals)
        self.updates += 1
        return True


class CountedGraph:
    """Stands for ops.CapturedGraph on the CPU: the launches run while they are 'captured', launch() does nothing.  What the
    tests look at is which graph object the cycle hands out and how many were made."""
    created = 0

    def __init__(self):
        type(self).created += 1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def launch(self):
        pass


def copy2d(src, dst, alpha=1.0, accumulate=False):
    _np(dst)[:] = alpha * _np(src) + (_np(dst) if accumulate else 0.0)
    return dst


def namespace():
    class Graph(CountedGraph):
        created = 0
    return C.block_namespace(shim, block_twin=Snapshot, CapturedGraph=Graph, copy2d=copy2d)


def hierarchy(levels=R.LEVELS, **kw):
    A1, _, hier, _ = R.problem(levels)
    # (a copy: on the CPU the hierarchy's fine matrix shares the memory of the array it is given, and rebuild_numeric writes it)
    return Hierarchy(A1.copy(), hier, "cpu", ops_mod=namespace(), **kw)


def new_values(which, levels=R.LEVELS):
    A1, A2 = R.problem(levels)[:2]
    return torch.from_numpy((A1 if which == 1 else A2).data.copy())


def run(bc, B, cycles=CYCLES):
    """use_columns, the right-hand sides, `cycles` cycles: the norms before each and after the last, and the iterate."""
    m = B.shape[1]
    bc.use_columns(m)
    bc.levels[0].b[:, :m] = torch.from_numpy(np.ascontiguousarray(B))
    norms = []
    for _ in range(cycles):
        norms.append(bc.residual_norms())
        bc.cycle(R.STEPS, R.OMEGA)
    norms.append(bc.residual_norms())
    return np.array(norms), bc.levels[0].x.numpy().copy()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the premise of the device tests ----------------------------------------------------------------------------------------
def test_the_second_set_of_values_is_what_the_device_tests_assume():
    A1, A2, hier, B = R.problem()
    assert A1.nnz == A2.nnz == 6855 and np.array_equal(A1.indptr, A2.indptr) and np.array_equal(A1.indices, A2.indices)
    move = np.abs(A2.data - A1.data).max() / np.abs(A1.data).max()
    h1, _ = R.reference(1)
    h2, _ = R.reference(2)
    assert np.array_equal(h1[0], h2[0])                                   # (x = 0: the norms of the right-hand sides)
    apart = np.abs(h2[1:] - h1[1:]) / np.maximum(h1[1:], h2[1:])
    end = h2[R.CYCLES] / h2[0]
    print("values move by %.3g |A1|max; histories apart by %.3g (cycle 1) .. %.3g (cycle 8), at least %.3g; A2 ends at %s"
          % (move, apart[0].max(), apart[-1].max(), apart.min(), end))
    assert move > 0.5
    assert (apart > 1e-3).all()                                           # every cycle from the first on, every column used
    assert (end < 1e-3).all() and (end > 1e-8).all()                      # converges, and no floor in sight
    assert (h2[2:] / h2[1:-1]).max() < 0.5                                # (from the second cycle on: 0.23 .. 0.33 per cycle)
    # a cycle made wholly of A1's operators does not solve A2 x = b: what staleness costs, against the tolerance
    stale = HoistedVCycle(A1, hier)
    for j in range(R.NCOLS):
        x = np.zeros(A1.shape[0])
        for _ in range(R.CYCLES):
            x = stale.cycle(x, B[:, j], "Jacobi", R.STEPS, R.OMEGA)
        left = np.linalg.norm(B[:, j] - A2 @ x)
        print("column %d: a cycle of A1's operators leaves %.3g of the A2 residual, the right one %.3g" % (j, left / h2[0, j], end[j]))
        assert left > 100.0 * h2[R.CYCLES, j]


def test_the_lagged_preconditioner_changes_the_cg_history_from_the_first_iteration():
    A, hier, B = C.problem()
    Al = R.with_values(A, R.lagged_values(A))
    assert np.array_equal(Al.indptr, A.indptr) and np.array_equal(Al.indices, A.indices) and abs(Al - Al.T).max() < 1e-12
    lag = HoistedVCycle(Al, hier)
    M = lambda v: lag.cycle(np.zeros(A.shape[0]), v, "Jacobi", C.STEPS, C.OMEGA)    # noqa: E731
    want, _ = C.reference("V")
    for j in range(R.NCOLS):
        t, _ = C.pcg_ref(A, B[:, j], M, 6)
        rel = t[1:7] / want[1:7, j]
        print("column %d: lagged / exact history %s, lagged ratios %s" % (j, np.round(rel, 2), np.round(t[2:] / t[1:-1], 3)))
        assert abs(rel[0] - 1.0) > 1e-3 and rel[3] > 100.0
        assert (t[2:] / t[1:-1] < 0.9).all()                                  # still a preconditioner: it contracts
        t8, _ = C.pcg_ref(A, B[:, j], M, C.ITERATIONS)
        assert t8[-1] < 0.1 * t8[0]                                           # (0.010 .. 0.028 after 8 iterations)


def test_the_lagged_preconditioner_changes_the_gmres_history_from_the_first_iteration():
    A, hier, B, _ = G.problem()
    lag = HoistedVCycle(R.with_values(A, R.lagged_values(A)), hier)
    M = lambda v: lag.cycle(np.zeros(A.shape[0]), v, "Jacobi", G.STEPS, G.OMEGA)    # noqa: E731
    _, want, _ = G.reference("V")
    for j in range(R.NCOLS):
        _, t, its = fgmres_ref(A, B[:, j], M, restart=G.RESTART, max_iterations=G.ITERATIONS, error=0.0)
        t = np.array(t)
        print("column %d: lagged / exact estimate of iteration 1: %.3g, end / start %.3g" % (j, t[1] / want[1, j], t[-1] / t[0]))
        assert its == G.ITERATIONS and abs(t[1] / want[1, j] - 1.0) > 1e-3    # (a factor 1.4 .. 2.1)
        assert t[-1] < 0.1 * t[0]                                             # (0.005 .. 0.062 after 10 iterations of GMRES(4))


# ---- the contract ---------------------------------------------------------------------------------------------------------
def test_the_stand_in_twin_is_a_copy_that_goes_stale():
    H = hierarchy()
    assert H.sizes == [1089, 289, 81] and H.coarse.kind == "dense"
    bc = BlockCycle(H, 3)
    before = [bl.A.vals.clone() for bl in bc.levels]
    H.rebuild_numeric(new_values(2))
    for bl, lev, old in zip(bc.levels, H.levels, before):
        assert bl.A is not lev.A and torch.equal(bl.A.vals, old) and not torch.equal(lev.A.vals, old)


def test_eager_cycle_after_a_rebuild():
    _, A2, hier, B = R.problem()
    H = hierarchy()
    bc = BlockCycle(H, 3)
    first = run(bc, B[:, :3], 2)                                          # warm buffers, the ping-pong has moved
    H.rebuild_numeric(new_values(2))
    old = run(bc, B[:, :3])
    new = run(BlockCycle(H, 3), B[:, :3])
    assert same(old, new)
    assert not np.array_equal(old[0][1], first[0][1])
    want, wx = R.reference(2, cycles=CYCLES)
    R.close(old[0], want)
    R.close_x(old[1][:, :3], wx)
    assert not old[1][:, 3].any()
    assert [bl.A.updates for bl in bc.levels] == [1, 1, 1]                # in place: the twins are the objects they were


class Refusing(Snapshot):
    """A twin of the matrix's own that refuses its new values: repack_values then puts another object -- here none -- in
    its place."""
    colmode = 1

    def update_values(self, A):
        return False


def test_a_twin_that_is_the_matrix_s_own_is_asked_for_again():
    """Levels 1 and 2 carry a twin of their own (A.sell), which is what block_twin then hands out and what repack_values
    refreshes: level 1's in place, level 2's by replacing it."""
    _, A2, hier, B = R.problem()
    H = hierarchy()
    H.ops.block_twin = lambda A: A.sell if getattr(A, "sell", None) is not None else Snapshot(A)
    H.levels[1].A.sell, H.levels[2].A.sell = Snapshot(H.levels[1].A), Refusing(H.levels[2].A)
    bc = BlockCycle(H, 3)
    assert [bl.A is lev.A.sell for bl, lev in zip(bc.levels, H.levels)] == [False, True, True]
    run(bc, B[:, :3], 2)
    was = [bl.A for bl in bc.levels]
    H.rebuild_numeric(new_values(2))
    assert H.levels[1].A.sell is was[1] and H.levels[2].A.sell is None
    old = run(bc, B[:, :3])
    assert [bl.A is w for bl, w in zip(bc.levels, was)] == [True, True, False]
    assert [bl.A.updates for bl in bc.levels] == [1, 1, 0]                # (level 1: by repack_values, not a second time)
    assert same(old, run(BlockCycle(H, 3), B[:, :3]))
    want, wx = R.reference(2, cycles=CYCLES)
    R.close(old[0], want)
    R.close_x(old[1][:, :3], wx)
    H.rebuild_numeric(new_values(1))                                      # level 2's twin is the cycle's own now
    assert same(run(bc, B[:, :3]), run(BlockCycle(H, 3), B[:, :3]))
    assert [bl.A.updates for bl in bc.levels] == [2, 2, 1]


def test_two_rebuilds_and_a_rebuild_nobody_looked_at():
    A1, A2, hier, B = R.problem()
    H = hierarchy()
    bc = BlockCycle(H, 3)
    H.rebuild_numeric(new_values(2))
    assert same(run(bc, B[:, :3]), run(BlockCycle(H, 3), B[:, :3]))
    H.rebuild_numeric(new_values(1))
    H.rebuild_numeric(new_values(2))                                      # (two rebuilds between two uses)
    H.rebuild_numeric(new_values(1))
    old = run(bc, B[:, :3])
    assert same(old, run(BlockCycle(H, 3), B[:, :3]))
    want, wx = R.reference(1, cycles=CYCLES)
    R.close(old[0], want)
    R.close_x(old[1][:, :3], wx)


@pytest.mark.parametrize("entry", ["cycle", "apply", "apply_graph", "residual_norms", "captured"])
def test_every_entry_point_notices_the_rebuild(entry):
    """The first call after the rebuild is `entry`, with no use_columns in between."""
    _, _, _, B = R.problem()
    H = hierarchy()
    bc = BlockCycle(H, 3)
    run(bc, B[:, :3], 1)
    H.rebuild_numeric(new_values(2))
    new = BlockCycle(H, 3)
    src = torch.zeros((1089, 4), dtype=torch.float64)
    src[:, :3] = torch.from_numpy(np.ascontiguousarray(B[:, :3]))
    for c in (bc, new):
        for t in (c.levels[0].x, c.levels[0].b):
            t.copy_(src)
    if entry == "cycle":
        got, want = (c.cycle(R.STEPS, R.OMEGA) or c.levels[0].x.clone() for c in (bc, new))
    elif entry in ("apply", "apply_graph"):
        got, want = (c.apply(src, None, R.STEPS, R.OMEGA, use_graph=entry == "apply_graph").clone() for c in (bc, new))
    elif entry == "residual_norms":
        got, want = (torch.tensor(c.residual_norms()) for c in (bc, new))
    else:
        got, want = (c.captured(R.STEPS, R.OMEGA) and c.levels[0].x.clone() for c in (bc, new))     # (the eager stand-in ran it)
    assert torch.equal(got, want) and bool(got.abs().max() > 0)


def test_a_captured_cycle_is_dropped_by_a_rebuild_and_by_nothing_else():
    H = hierarchy()
    Graph = H.ops.CapturedGraph
    bc = BlockCycle(H, 3)
    g = bc.captured(R.STEPS, R.OMEGA, "V")
    w = bc.captured(R.STEPS, R.OMEGA, "W")
    assert Graph.created == 2 and g is not w
    assert bc.captured(R.STEPS, R.OMEGA, "V") is g and bc.captured(R.STEPS, R.OMEGA, "W") is w
    bc.use_columns(3)
    bc.cycle(R.STEPS, R.OMEGA)
    bc.residual_norms()
    assert bc.captured(R.STEPS, R.OMEGA, "V") is g and Graph.created == 2
    H.rebuild_numeric(new_values(2))
    g2 = bc.captured(R.STEPS, R.OMEGA, "V")
    assert g2 is not g and Graph.created == 3
    assert bc.captured(R.STEPS, R.OMEGA, "V") is g2 and Graph.created == 3
    assert bc.captured(R.STEPS, R.OMEGA, "W") is not w and Graph.created == 4
    # apply(use_graph=True) goes through the same cache
    src = torch.ones((1089, 4), dtype=torch.float64)
    bc.apply(src, None, R.STEPS, R.OMEGA, use_graph=True)
    assert Graph.created == 4
    H.rebuild_numeric(new_values(1))
    bc.apply(src, None, R.STEPS, R.OMEGA, use_graph=True)
    assert Graph.created == 5


def test_column_loop_over_a_coarse_solver_without_a_block_form():
    _, A2, hier, B = R.problem(2)
    H = hierarchy(2, coarse_solver="banded", coarse_refine=1)
    assert H.coarse.kind == "banded-block" and H.sizes == [1089, 289]
    bc = BlockCycle(H, 3)
    assert not bc.dense_coarse
    run(bc, B[:, :3], 2)
    H.rebuild_numeric(new_values(2, 2))
    assert H.coarse.kind == "banded-block"
    old = run(bc, B[:, :3])
    assert same(old, run(BlockCycle(H, 3), B[:, :3]))
    want, wx = R.reference(2, 2, cycles=CYCLES)
    R.close(old[0], want)
    R.close_x(old[1][:, :3], wx)


@pytest.mark.parametrize("first,then", [("dense", "banded"), ("banded", "dense")])
def test_dense_coarse_follows_a_coarse_solver_that_changed_kind(first, then):
    """_factor_coarsest replaces H.coarse where factor() refuses the new operator: the refusal is staged here (factor raises
    the ValueError it raises for a pattern it does not know), the replacement is the hierarchy's own."""
    kinds = {"dense": "dense", "banded": "banded-block"}
    _, A2, hier, B = R.problem(2)
    H = hierarchy(2, coarse_solver=first)
    assert H.coarse.kind == kinds[first]
    bc = BlockCycle(H, 3)
    assert bc.dense_coarse == (first == "dense")
    run(bc, B[:, :3], 1)

    def refuse(A):
        raise ValueError("coarse operator changed its sparsity pattern")

    H.coarse.factor = refuse
    H.coarse_strategy = then
    H.rebuild_numeric(new_values(2, 2))
    assert H.coarse.kind == kinds[then]
    old = run(bc, B[:, :3])
    assert bc.dense_coarse == (then == "dense")
    assert bc.dense_coarse or (bc.col_b is not None and bc.col_x is not None)
    assert same(old, run(BlockCycle(H, 3), B[:, :3]))
    want, wx = R.reference(2, 2, cycles=CYCLES)
    R.close(old[0], want)
    R.close_x(old[1][:, :3], wx)
