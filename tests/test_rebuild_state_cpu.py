"""Hierarchy.rebuild_numeric() state by state against a fresh hierarchy, without a GPU: the bookkeeping of
tests/test_rebuild_state_gpu.py through the CPU stand-in of the ops module (tests/cpu_ops_shim.py), which has no storage twins.
After one, two and three rebuilds of one hierarchy the coarse operators, the inverse diagonals, the Chebyshev bounds and tables,
the line factors, the coarse factors, `generation` and the captured cycles are those of a hierarchy built from the new values
(tests/rebuild_cases.py: assert_same_state), and a smoother prepared after a rebuild equals one prepared before it and renewed."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cpu_ops_shim as shim
import rebuild_cases as R
from learnmultigrid_amd.hierarchy import Hierarchy

# name -> (elements per side, the value sets).  The Line smoother runs on the 33^2 grid: without grid twins a level of 4096 rows
# or more has no line geometry (Hierarchy._line_stride reads the pattern of smaller levels on the host).
CHAINS = {"grid-kinds-change": (R.M, ("const", "var45", "const", "var45")),
          "grid-kinds-stay": (R.M, ("var44", "var45", "var44", "var45")),
          "learned": (R.M, ("jit", "jit45", "jit", "jit45")),
          "grid-33-line": (32, ("const", "var45", "const", "var44"))}
CHEBY = R.CONFIGS["cheby-3"]
JACOBI = R.CONFIGS["jacobi-W"]
GS = R.CONFIGS["gs-lex-forward"]


class EagerGraph:
    """Stands for ops.CapturedGraph on the CPU: the launches run while they are 'captured', launch() does nothing."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def launch(self):
        pass


def hierarchy(name, m=R.M, **kw):
    # (a copy: on the CPU the hierarchy's fine matrix shares the memory of the array it is given, and rebuild_numeric writes it)
    return Hierarchy(R.matrix(name, m).copy(), list(R.transfers(name, m)), "cpu", ops_mod=shim.namespace(CapturedGraph=EagerGraph),
                     **kw)


def configs(m=R.M):
    return [JACOBI, CHEBY, GS] + ([R.LINE_CONFIG] if m == 32 else [])


def prepare(H, cfgs):
    for smoother, _steps, _omega, gs_mode, gs_sweep, _shape, kw in cfgs:
        H.prepare_smoother(smoother, gs_mode, gs_sweep=gs_sweep, **kw)


def cycle(H, cfg):
    smoother, steps, omega, gs_mode, gs_sweep, shape, kw = cfg
    H.levels[0].b.copy_(torch.from_numpy(R.rhs(H.levels[0].n).copy()))
    H.cycle(smoother, steps, omega, gs_mode, x_is_zero=True, gs_sweep=gs_sweep, shape=shape, **kw)
    return H.levels[0].x.clone()


def capture(H, cfg):
    smoother, steps, omega, gs_mode, gs_sweep, shape, kw = cfg
    return H.captured_cycle(smoother, steps, omega, gs_mode, gs_sweep=gs_sweep, shape=shape, **kw)


def test_the_value_sets_are_what_the_device_tests_assume():
    for name in R.SCENARIOS:
        mats, hier, _ = R.scenario(name)
        assert [q.shape for q in hier] == [(4225, 1089), (1089, 289)]
        assert all(A.nnz == mats[0].nnz for A in mats)
    const, var44, var45 = (R.matrix(v) for v in ("const", "var44", "var45"))
    assert const.nnz == var45.nnz == 20101
    assert [np.unique(A.data).size for A in (const, var44, var45)] == [3, 12034, 12034]
    assert R.matrix("jit").nnz == R.matrix("jit45").nnz == 28039
    for a, b in (("const", "var45"), ("var44", "var45"), ("jit", "jit45")):
        move = np.abs(R.matrix(a).data - R.matrix(b).data).max() / np.abs(R.matrix(a).data).max()
        print("%s -> %s: the values move by %.3g of the largest" % (a, b, move))
        assert move > 0.1


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_state_after_one_two_and_three_rebuilds(chain):
    m, names = CHAINS[chain]
    cfgs = configs(m)
    H = hierarchy(names[0], m)
    assert H.sizes == (R.SIZES if m == R.M else [1089, 289, 81]) and H.generation == 0
    prepare(H, cfgs)
    before = [cycle(H, cfg) for cfg in cfgs]                              # (the Jacobi cycle makes level 0's dinv on the way)
    assert H.levels[0].dinv is not None
    for k, name in enumerate(names[1:], start=1):
        graphs = [capture(H, cfg) for cfg in cfgs]
        assert len(H._graphs) == len(cfgs) and all(capture(H, cfg) is g for cfg, g in zip(cfgs, graphs))
        H.rebuild_numeric(R.values(R.matrix(name, m)))
        assert H.generation == k and H._graphs == {}
        F = hierarchy(name, m)
        prepare(F, cfgs)
        R.assert_same_state(H, F)
        after = [cycle(H, cfg) for cfg in cfgs]
        fresh = [cycle(F, cfg) for cfg in cfgs]
        for cfg, x, xf, x0 in zip(cfgs, after, fresh, before):
            assert torch.equal(x, xf), (k, cfg[0])
            assert not torch.equal(x, x0), (k, cfg[0])
        R.assert_same_state(H, F)                                          # (the tables and schedules the cycles made lazily)
        assert all(capture(H, cfg) is not g for cfg, g in zip(cfgs, graphs))
        before = after


def test_a_rebuild_with_the_same_values_changes_nothing_but_the_generation():
    cfgs = configs(32)
    H = hierarchy("const", 32)
    prepare(H, cfgs)
    before = [cycle(H, cfg) for cfg in cfgs]
    capture(H, JACOBI)
    H.rebuild_numeric(R.values(R.matrix("const", 32)))
    assert H.generation == 1 and H._graphs == {}
    F = hierarchy("const", 32)
    prepare(F, cfgs)
    R.assert_same_state(H, F)
    assert all(torch.equal(cycle(H, cfg), x0) for cfg, x0 in zip(cfgs, before))


def test_a_smoother_prepared_after_the_rebuild_equals_one_prepared_before_it_and_renewed():
    cfgs = configs(32)
    early, late = hierarchy("const", 32), hierarchy("const", 32)
    prepare(early, cfgs)
    assert late.cheby_key() is None and late.line_key() is None
    for H in (early, late):
        H.rebuild_numeric(R.values(R.matrix("var45", 32)))
    assert late.cheby_key() is None and late.line_key() is None           # nothing was prepared: nothing is renewed
    assert all(lev.line is None for lev in late.levels)
    prepare(late, cfgs)
    R.assert_same_state(early, late)
    for cfg in cfgs:
        assert torch.equal(cycle(early, cfg), cycle(late, cfg)), cfg[0]
    # overrides in use survive the rebuild: the bounds that were given are not replaced by Gershgorin's
    H = hierarchy("const", 32)
    H.prepare_smoother("Chebyshev", cheby_lmax=[1.9, 1.7], cheby_ratio=8.0)
    H.prepare_smoother("Line", line_dir="y", line_order="jacobi")
    H.rebuild_numeric(R.values(R.matrix("var45", 32)))
    assert H.cheby_key() == ((1.9, 1.7), 8.0) and H.line_key() == ("y", "jacobi")
    F = hierarchy("var45", 32)
    F.prepare_smoother("Chebyshev", cheby_lmax=[1.9, 1.7], cheby_ratio=8.0)
    F.prepare_smoother("Line", line_dir="y", line_order="jacobi")
    R.assert_same_state(H, F)


def test_a_wrong_number_of_values_raises_and_changes_nothing():
    H = hierarchy("const")
    prepare(H, [CHEBY])
    g = capture(H, CHEBY)
    was = [lev.A.vals.clone() for lev in H.levels]
    key = H.cheby_key()
    for numel in (R.matrix("const").nnz - 1, R.matrix("const").nnz + 1, 0):
        with pytest.raises(ValueError):
            H.rebuild_numeric(torch.ones(numel, dtype=torch.float64))
    assert H.generation == 0 and capture(H, CHEBY) is g and H.cheby_key() == key
    assert all(torch.equal(lev.A.vals, v) for lev, v in zip(H.levels, was))


def test_mass_and_operator_rebuilds_do_not_disturb_each_other():
    """The mass-like matrix of test_mass_matrix_coarsening_on_the_device (tests/test_solvers_gpu.py): random values on the
    operator's pattern.  The two products run through plans of their own."""
    A = R.matrix("const")
    rng = np.random.default_rng(3)
    M1, M2 = (sp.csr_matrix((rng.random(A.nnz) + 0.1, A.indices.copy(), A.indptr.copy()), shape=A.shape) for _ in range(2))
    hier = list(R.transfers("const"))
    H = Hierarchy(A.copy(), hier, "cpu", ops_mod=shim.namespace(), mass=M1.copy())

    def masses(G):
        return [lev.M.vals.clone() for lev in G.levels]

    def operators(G):
        return [lev.A.vals.clone() for lev in G.levels]

    def same(a, b):
        return all(torch.equal(u, v) for u, v in zip(a, b))

    m1 = masses(H)
    H.rebuild_numeric(R.values(R.matrix("var45")))
    assert same(masses(H), m1) and H.generation == 1
    a45 = operators(H)
    H.rebuild_mass_numeric(torch.from_numpy(M2.data.copy()))
    assert same(operators(H), a45) and H.generation == 1                  # (generation counts the operator's rebuilds)
    F = Hierarchy(R.matrix("var45").copy(), hier, "cpu", ops_mod=shim.namespace(), mass=M2.copy())
    assert same(masses(H), masses(F)) and not same(masses(H)[1:], m1[1:])
    R.assert_same_state(H, F)
    H.rebuild_numeric(R.values(A))                                        # the replay path, with the new mass in place
    assert same(masses(H), masses(F))
    R.assert_same_state(H, Hierarchy(A.copy(), hier, "cpu", ops_mod=shim.namespace()))
    with pytest.raises(ValueError):
        H.rebuild_mass_numeric(torch.ones(A.nnz - 1, dtype=torch.float64))
    with pytest.raises(ValueError):
        Hierarchy(A.copy(), hier, "cpu", ops_mod=shim.namespace()).rebuild_mass_numeric(torch.from_numpy(M2.data.copy()))
