"""Block cycles across Hierarchy.rebuild_numeric() (-m gpu): a block.BlockCycle built BEFORE the rebuild -- directly, or
cached inside Multigrid / CG / GMRES.solve_many -- must give the bits of one built AFTER it on the same rebuilt hierarchy, and
both must follow the CPU oracle on the new values at the project's history tolerance.  A BlockCycle holds state of its own
that the hierarchy does not see: sliced-ELL twins that are copies of a level's values, captured hipGraphs with the address of
the old coarse inverse in them, and which kind of coarse solver there is.

The problem is the one of tests/test_block_cycle_gpu.py (33^2 jittered operator, 1089 -> 289 -> 81, V(2, 2) at omega = 0.8,
8 cycles); the second set of values, A2, has a log-normal element coefficient on the same pattern (tests/block_rebuild_ref.py).
What makes a stale cycle visible is asserted without a device in tests/test_block_rebuild_cpu.py: the oracle histories of A1
and A2 are 0.22 .. 0.97 apart in every cycle, A2's ends at 1e-5 .. 3e-4 of its start, a cycle of A1's operators leaves 0.5 .. 3.8
of it -- nine orders and more above RTOL = 1e-10."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import block_cg_ref as CGR                                           # noqa: E402
import block_gmres_ref as GMR                                        # noqa: E402
import block_rebuild_ref as R                                        # noqa: E402
import test_block_cycle_gpu as T                                     # noqa: E402  (its problem and its oracle on A1)
from learnmultigrid_amd import ops                                   # noqa: E402
from learnmultigrid_amd.block import BlockCycle                      # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy                   # noqa: E402
from learnmultigrid_amd.solvers import CG, GMRES, HierarchyMG        # noqa: E402
from support import DEV, dev                                         # noqa: E402

CYCLES, STEPS, OMEGA = R.CYCLES, R.STEPS, R.OMEGA
close, close_x = R.close, R.close_x


def hierarchy(levels=R.LEVELS, **kw):
    A1, _, hier, _ = R.problem(levels)
    H = Hierarchy(A1, hier, DEV, **kw)
    torch.cuda.synchronize()                                           # (built on the current stream, used on H.stream)
    return H


def rebuild(H, which, levels=R.LEVELS):
    A1, A2 = R.problem(levels)[:2]
    H.rebuild_numeric(dev((A1 if which == 1 else A2).data))


def run(bc, B, cycles=CYCLES, shape="V", graph=False):
    """use_columns, the right-hand sides, `cycles` cycles (graph: replays of the captured cycle): the norms before each cycle
    and the last iterate.  On H.stream (the caller's `with`)."""
    m = B.shape[1]
    bc.use_columns(m)
    bc.levels[0].b[:, :m].copy_(dev(B))
    g = bc.captured(STEPS, OMEGA, shape) if graph else None
    norms = []
    for _ in range(cycles):
        norms.append(bc.residual_norms())
        if g is not None:
            g.launch()
        else:
            bc.cycle(STEPS, OMEGA, shape)
    return np.array(norms), bc.levels[0].x.cpu().numpy()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def against_oracle(got, want, cycles=CYCLES):
    hist, X = want
    close(got[0], hist[:cycles])
    close_x(got[1][:, :R.NCOLS], X)
    assert not got[1][:, R.NCOLS:].any()                               # the padding column stays zero


def test_level_0_has_a_twin_of_the_block_cycles_own():
    """6855 entries in 1089 rows are fewer than ops.SELL_MIN_AVG = 12 a row: pack() gives level 0 no sliced-ELL twin and
    the block cycle builds one from a copy of the values -- the twin a rebuild cannot reach, and what makes the tests below
    say something.  On the device levels 1 (289 rows of up to 25 entries) and 2 (81 rows of up to 49) turned out to hold a
    twin of the cycle's own as well: all three levels are private (printed below, not asserted)."""
    H = hierarchy()
    assert H.sizes == [1089, 289, 81] and H.coarse.kind == "dense"
    with torch.cuda.stream(H.stream):
        bc = BlockCycle(H, 3)
    torch.cuda.synchronize()
    assert bc.levels[0].A is not H.levels[0].A.sell
    print("block twin shared with the level's matrix, per level:", [bl.A is lev.A.sell for bl, lev in zip(bc.levels, H.levels)])


def test_eager_cycle_after_a_rebuild():
    B = R.problem()[3][:, :3]
    H = hierarchy()
    with torch.cuda.stream(H.stream):
        bc = BlockCycle(H, 3)
        run(bc, B, 2)                                                  # warm buffers, the ping-pong has moved
        rebuild(H, 2)
        old = run(bc, B)
        new = run(BlockCycle(H, 3), B)
    torch.cuda.synchronize()
    assert same(old, new)
    against_oracle(old, R.reference(2))


def test_levels_whose_block_twin_is_the_matrix_s_own():
    """pack() gives none of the three levels a sliced-ELL twin here (it does on larger levels with rows this long).  Levels 1
    and 2 are handed one, the way tests/test_block_sweeps_gpu.py does: the block cycle then reads the twin rebuild_numeric
    refreshes itself (repack_values), and asks for it again after a rebuild."""
    B = R.problem()[3][:, :3]
    H = hierarchy()
    for lev in H.levels[1:]:
        assert lev.A.sell is None
        lev.A.sell = ops.SellCSR.from_csr(lev.A, max_padding=float("inf"))
        assert lev.A.sell is not None and ops.block_twin(lev.A) is lev.A.sell
    with torch.cuda.stream(H.stream):
        bc = BlockCycle(H, 3)
        assert [bl.A is lev.A.sell for bl, lev in zip(bc.levels, H.levels)] == [False, True, True]
        run(bc, B, 2)
        rebuild(H, 2)
        old = run(bc, B)
        assert [bl.A is lev.A.sell for bl, lev in zip(bc.levels, H.levels)] == [False, True, True]
        new = run(BlockCycle(H, 3), B)
    torch.cuda.synchronize()
    assert same(old, new)
    against_oracle(old, R.reference(2))


def test_two_rebuilds():
    """A1 -> A2 -> A1: one rebuild sorts and records the SpGEMM map, the next replays it."""
    B = R.problem()[3][:, :3]
    H = hierarchy()
    with torch.cuda.stream(H.stream):
        bc = BlockCycle(H, 3)
        run(bc, B, 2)
        rebuild(H, 2)
        old2 = run(bc, B)
        new2 = run(BlockCycle(H, 3), B)
        rebuild(H, 1)
        old1 = run(bc, B)
        new1 = run(BlockCycle(H, 3), B)
    torch.cuda.synchronize()
    assert same(old2, new2) and same(old1, new1)
    against_oracle(old2, R.reference(2))
    hist, Xs = T.reference()
    against_oracle(old1, (hist[:, :3], Xs[CYCLES][:, :3]))


@pytest.mark.parametrize("shape,cycles", [("V", CYCLES), ("W", 3)])
def test_captured_cycle_after_a_rebuild(shape, cycles):
    B = R.problem()[3][:, :3]
    H = hierarchy()
    with torch.cuda.stream(H.stream):
        bc = BlockCycle(H, 3)
        bc.use_columns(3)
        bc.levels[0].b[:, :3].copy_(dev(B))
        g = bc.captured(STEPS, OMEGA, shape)
        g.launch()
        assert bc.captured(STEPS, OMEGA, shape) is g
        rebuild(H, 2)
        g2 = bc.captured(STEPS, OMEGA, shape)
        assert g2 is not g
        old = run(bc, B, cycles, shape, graph=True)
        assert bc.captured(STEPS, OMEGA, shape) is g2                  # not captured again without a rebuild
        new = run(BlockCycle(H, 3), B, cycles, shape)
    torch.cuda.synchronize()
    assert same(old, new)
    if shape == "V":
        against_oracle(old, R.reference(2))


@pytest.mark.parametrize("use_graph", [False, True])
def test_apply_as_a_preconditioner_after_a_rebuild(use_graph):
    B = R.problem()[3]
    src = np.zeros((B.shape[0], 4))
    src[:, :3] = B[:, 3:6]
    H = hierarchy()
    with torch.cuda.stream(H.stream):
        bc = BlockCycle(H, 3)
        s, dst = dev(src), torch.zeros((B.shape[0], 4), dtype=torch.float64, device=DEV)
        before = bc.apply(s, dst, STEPS, OMEGA, use_graph=use_graph).cpu().numpy()
        assert np.array_equal(dst.cpu().numpy(), before)
        rebuild(H, 2)
        old = bc.apply(s, dst, STEPS, OMEGA, use_graph=use_graph).cpu().numpy()
        assert np.array_equal(dst.cpu().numpy(), old)
        new = BlockCycle(H, 3).apply(s, None, STEPS, OMEGA).cpu().numpy()
    torch.cuda.synchronize()
    assert np.array_equal(old, new)
    assert np.abs(old - before).max() > 1e-3 * np.abs(before).max()    # the sensitivity: the other operator is another cycle


@pytest.mark.parametrize("refine", [0, 1])
def test_column_loop_over_a_coarse_solver_without_a_block_form(refine):
    """Two levels, 1089 -> 289, where the banded solver builds (tests/test_block_cycle_gpu.py): the column vectors, and the
    numeric phase of a Schur solver across a rebuild."""
    B = R.problem(2)[3][:, :3]
    H = hierarchy(2, coarse_solver="banded", coarse_refine=refine)
    assert H.coarse.kind == "banded-block" and H.sizes == [1089, 289]
    with torch.cuda.stream(H.stream):
        bc = BlockCycle(H, 3)
        assert bc.k == 4 and not bc.dense_coarse
        run(bc, B, 2)
        rebuild(H, 2, 2)
        assert H.coarse.kind == "banded-block"
        old = run(bc, B)
        new = run(BlockCycle(H, 3), B)
    torch.cuda.synchronize()
    assert same(old, new)
    against_oracle(old, R.reference(2, 2))


# ---- through the solvers: their caches are keyed on the identity of the hierarchy, which a rebuild does not change ---------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_multigrid_solve_many_after_a_rebuild(use_graph):
    """solve_many takes its residual norms with the block twin of level 0: after the rebuild the history is the oracle's on
    A2, whatever matrix the solver object was given."""
    A1, rhs, hier, B = T.problem()
    A2 = R.problem()[1]
    mg = HierarchyMG(A1, rhs.copy(), hier)
    _, t1 = mg.solve_many(B[:, :3], max_iterations=CYCLES, use_graph=use_graph, **T.KW)
    close(t1, T.reference()[0][:CYCLES, :3])
    H = mg._hier
    with torch.cuda.stream(H.stream):
        H.rebuild_numeric(dev(A2.data))
    torch.cuda.synchronize()
    X, track = mg.solve_many(B[:, :3], max_iterations=CYCLES, use_graph=use_graph, **T.KW)
    assert mg._hier is H
    hist, X2 = R.reference(2)
    close(track, hist[:CYCLES])
    close_x(X, X2)
    X3, track3 = mg.solve_many(B[:, :3], max_iterations=CYCLES, use_graph=not use_graph, **T.KW)
    assert np.array_equal(X, X3) and np.array_equal(track, track3)


def lagged_preconditioner(make, A, hier, B, use_graph, **kw):
    """The solver keeps its matrix; its preconditioner is rebuilt on A + 0.1 diag(A) (same pattern: a lagged preconditioner).
    Returns the runs before the rebuild, after it on the same solver object, and on a new solver object."""
    H = Hierarchy(A, hier, DEV)
    assert H.sizes == [1089, 289, 81] and H.coarse.kind == "dense"
    kw = dict(kw, error=0.0, preconditioner=H, use_graph=use_graph)
    solver = make()
    before = solver.solve_many(B, **kw)
    with torch.cuda.stream(H.stream):
        H.rebuild_numeric(dev(R.lagged_values(A)))
    torch.cuda.synchronize()
    old = solver.solve_many(B, **kw)
    new = make().solve_many(B, **kw)
    other = solver.solve_many(B, **dict(kw, use_graph=not use_graph))
    assert np.array_equal(old[0], other[0]) and np.array_equal(old[1], other[1])
    return before, old, new


@pytest.mark.parametrize("use_graph", [False, True])
def test_cg_solve_many_with_a_preconditioner_rebuilt_under_it(use_graph):
    """tests/test_block_rebuild_cpu.py: the lagged preconditioner moves the recurrence norm of iteration 1 by a factor
    2.6 .. 3.0 and still contracts."""
    A, hier, B = CGR.problem()
    before, old, new = lagged_preconditioner(lambda: CG(A, B[:, :1].copy()), A, hier, B[:, :3], use_graph,
                                             max_iterations=CGR.ITERATIONS, precond_steps=CGR.STEPS, precond_omega=CGR.OMEGA)
    assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1])
    assert np.array_equal(old[1][0], before[1][0])                     # (row 0: the true norms of the zero guess)
    assert (np.abs(old[1][1] / before[1][1] - 1.0) > 1e-3).all()
    assert (old[1][-1] < 0.1 * old[1][0]).all()                        # still a preconditioner: 0.010 .. 0.028 of the start after 8


@pytest.mark.parametrize("use_graph", [False, True])
def test_gmres_solve_many_with_a_preconditioner_rebuilt_under_it(use_graph):
    """tests/test_block_rebuild_cpu.py: here the lagged preconditioner moves the first estimate by a factor 1.4 .. 2.1, and
    10 iterations of GMRES(4) end at 0.005 .. 0.062 of the start."""
    A, hier, B, _ = GMR.problem()
    before, old, new = lagged_preconditioner(lambda: GMRES(A, B[:, :1].copy()), A, hier, B[:, :3], use_graph,
                                             max_iterations=GMR.ITERATIONS, restart=GMR.RESTART, precond_steps=GMR.STEPS,
                                             precond_omega=GMR.OMEGA)
    assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1])
    assert np.array_equal(old[1][0], before[1][0])
    assert (np.abs(old[1][1] / before[1][1] - 1.0) > 1e-3).all()
    assert (old[1][-1] < 0.1 * old[1][0]).all()
