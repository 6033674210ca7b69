"""Hierarchy.rebuild_numeric() state by state against a fresh hierarchy (-m gpu), scenario by smoother configuration
(tests/rebuild_cases.py: the 65^2 grid, 4225 -> 1089 -> 289).  Every test

  1. prepares the smoother on the first set of values, runs one eager cycle from a zero iterate on a seeded right-hand side,
     takes the captured cycle and replays it once -- all lazy state now exists on the old values;
  2. rebuilds (the round trip: through every set of values, with step 1 on each);
  3. compares the state with that of F = Hierarchy(last values, the same transfers) after the same prepare_smoother call
     (rebuild_cases.assert_same_state: CSR arrays, inverse diagonals, which twins there are, every twin against the plain CSR
     sweeps, the coarse solver, Chebyshev tables, line factors);
  4. runs the eager cycle and a replay of the captured cycle, which must be a new graph, on both, and compares the iterates.

Where the rebuilt hierarchy has the twin kinds of the fresh one the iterates are equal bit for bit.  They are asserted equal
bit for bit in var44 -> const too, where the kinds differ (below): the project claims that every path has the bits of the
separate sweeps.  A configuration for which that turns out not to hold is listed in NOT_BITWISE_ACROSS_KINDS with what was
measured, and held to the project's bound for cycles (1e-10 relative, floor 1e-14 ||b||) instead.

var44 -> const: a hierarchy built on per-row values has packed CSR twins (level 0: and the DIA twin) on every level, and
DeviceCSR.repack_values() keeps the formats a matrix has: it re-encodes their value streams and only builds other twins where
one of them refuses the new values.  The three values of the constant-coefficient operator fit every format, so the rebuilt
hierarchy stays on packed CSR and DIA, while a fresh one gets row patterns with their stencil view (limits).  The
kinds of both are printed; every twin must still hold the new values."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rebuild_cases as R                                            # noqa: E402
from learnmultigrid_amd.block import BlockCycle                      # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy                   # noqa: E402
from support import DEV, dev                                         # noqa: E402

# (scenario, configuration) -> the largest deviation measured, in units of the bound for cycles (rebuild_cases.within_cycle_bound)
NOT_BITWISE_ACROSS_KINDS = {}


def hierarchy(A, hier, **kw):
    H = Hierarchy(A.copy(), list(hier), DEV, **kw)
    torch.cuda.synchronize()                                           # (built on the current stream, used on H.stream)
    return H


def prepare(H, cfg):
    smoother, _steps, _omega, gs_mode, gs_sweep, _shape, kw = cfg
    with torch.cuda.stream(H.stream):
        H.prepare_smoother(smoother, gs_mode, gs_sweep=gs_sweep, **kw)
    torch.cuda.synchronize()


def rebuild(H, A):
    vals = dev(A.data)
    with torch.cuda.stream(H.stream):
        H.rebuild_numeric(vals)
    torch.cuda.synchronize()


def run(H, cfg, b):
    """One eager cycle from a zero iterate, then one replay of the captured cycle: (iterate after the first, after the
    second, the graph)."""
    smoother, steps, omega, gs_mode, gs_sweep, shape, kw = cfg
    with torch.cuda.stream(H.stream):
        H.levels[0].b.copy_(b)
        H.cycle(smoother, steps, omega, gs_mode, x_is_zero=True, gs_sweep=gs_sweep, shape=shape, **kw)
        x1 = H.levels[0].x.clone()
        g = H.captured_cycle(smoother, steps, omega, gs_mode, gs_sweep=gs_sweep, shape=shape, **kw)
        assert H.captured_cycle(smoother, steps, omega, gs_mode, gs_sweep=gs_sweep, shape=shape, **kw) is g
        g.launch()
        x2 = H.levels[0].x.clone()
    torch.cuda.synchronize()
    H.check_smoothers()
    assert bool(torch.isfinite(x1).all()) and bool(torch.isfinite(x2).all()) and not torch.equal(x1, x2)
    return x1, x2, g


def check(name, label, cfg):
    mats, hier, same_kinds = R.scenario(name)
    b = dev(R.rhs())
    b_norm = float(np.linalg.norm(R.rhs()))
    H = hierarchy(mats[0], hier)
    assert H.sizes == R.SIZES and H.generation == 0
    prepare(H, cfg)
    before = run(H, cfg, b)
    graphs = [before[2]]
    for k, A in enumerate(mats[1:], start=1):
        rebuild(H, A)
        assert H.generation == k and H._graphs == {}
        if k < len(mats) - 1:
            graphs.append(run(H, cfg, b)[2])                           # lazy state on every set of values on the way
    F = hierarchy(mats[-1], hier)
    prepare(F, cfg)
    kinds = R.assert_same_state(H, F, same_kinds)
    after = run(H, cfg, b)
    assert all(after[2] is not g for g in graphs)
    fresh = run(F, cfg, b)
    R.assert_same_state(H, F, same_kinds)                              # (with what the cycles made lazily)
    assert H.generation == len(mats) - 1 and len(H._graphs) == 1
    exact = torch.equal(after[0], fresh[0]) and torch.equal(after[1], fresh[1])
    if not same_kinds:
        worst = max(R.within_cycle_bound(after[i], fresh[i], b_norm) for i in (0, 1))
        print("%s, %s: twins of A per level, rebuilt %s, fresh %s; iterates %s, deviation %.3g of the bound for cycles"
              % (name, label, [k[0] for k in kinds[0]], [k[0] for k in kinds[1]], "bitwise" if exact else "NOT bitwise", worst))
        if (name, label) in NOT_BITWISE_ACROSS_KINDS:
            assert worst <= 1.0, worst
            exact = True
    assert exact, (name, label)
    if mats[-1] is mats[0] and len(mats) == 2:
        assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])   # the same values: the same bits
    else:
        assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])
    return H, F, kinds


@pytest.mark.parametrize("label", sorted(R.CONFIGS))
@pytest.mark.parametrize("name", sorted(R.SCENARIOS))
def test_rebuilt_state_and_cycles_equal_a_fresh_hierarchy_s(name, label):
    check(name, label, R.CONFIGS[label])


@pytest.mark.parametrize("name", R.LINE_SCENARIOS)
def test_line_smoother_after_a_rebuild(name):
    H, _, _ = check(name, "line-x-zebra", R.LINE_CONFIG)
    assert H.line_key() == ("x", "zebra")


def test_which_twins_a_rebuild_changes_and_which_it_keeps():
    """const -> var45: the row patterns stop repeating, pack() starts over and level 0 gets packed CSR and DIA like a fresh
    hierarchy.  var44 -> const: the formats stay (the module docstring), level 0 keeps packed CSR and DIA where a fresh
    hierarchy has row patterns and their stencil view."""
    for name, rebuilt, fresh in (("const-var45", ("packed", "dia"), ("packed", "dia")),
                                 ("var44-const", ("packed", "dia"), ("patterns", "stencil"))):
        mats, hier, same_kinds = R.scenario(name)
        H = hierarchy(mats[0], hier)
        was = R.level_kinds(H)
        rebuild(H, mats[1])
        F = hierarchy(mats[1], hier)
        kinds = R.assert_same_state(H, F, same_kinds)
        print("%s: (A, P, R) twins per level before %s, rebuilt %s, fresh %s" % (name, was, kinds[0], kinds[1]))
        assert kinds[0][0][0] == rebuilt and kinds[1][0][0] == fresh
        assert "dia" not in kinds[0][1][0] and "dia" not in kinds[1][1][0]        # 1089 rows: below DiaTwin.MIN_ROWS


def test_fp32_twins_flip_their_width_with_the_range_rule_and_come_back():
    """cycle_values="f32" on the jittered pair.  The second set of values has one entry of 1e-50, which rounds to zero in
    fp32: the range rule refuses it, level 0 gets fp64 twins as a whole (DeviceCSR._retarget: pack() from scratch) and fp32
    twins again with the third set.  At either step state and iterates are those of a fresh cycle_values="f32" hierarchy."""
    cfg = R.CONFIGS["jacobi-V"]
    jit, jit45, hier = R.matrix("jit"), R.matrix("jit45"), R.transfers("jit")
    odd = jit45.copy()
    row = 32 * 65 + 32
    k = int(odd.indptr[row])
    assert odd.indices[k] != row and odd.data[k] != 0.0
    odd.data[k] = 1e-50
    b = dev(R.rhs())
    H = hierarchy(jit, hier, cycle_values="f32")
    assert [lev.A.twin_values for lev in H.levels] == ["f32"] * 3
    prepare(H, cfg)
    last = run(H, cfg, b)
    widths = []
    for step, A in enumerate((odd, jit45), start=1):
        rebuild(H, A)
        assert H.generation == step and H._graphs == {}
        F = hierarchy(A, hier, cycle_values="f32")
        prepare(F, cfg)
        R.assert_same_state(H, F)
        after, fresh = run(H, cfg, b), run(F, cfg, b)
        R.assert_same_state(H, F)
        assert after[2] is not last[2]
        assert torch.equal(after[0], fresh[0]) and torch.equal(after[1], fresh[1])
        assert not torch.equal(after[0], last[0]) and not torch.equal(after[1], last[1])
        widths.append([(lev.A.twin_values, R.twin_widths(lev.A)) for lev in H.levels])
        last = after
    print("what the twins of A hold per level, with the value out of range and without:", widths)
    assert widths[0][0][0] == "f64" and all(w == "f64" for w in widths[0][0][1].values())
    assert all(tv == "f32" and all(w == "f32" for w in tw.values()) for tv, tw in widths[1])


def test_a_block_cycle_made_before_the_rebuild_gives_the_columns_of_one_made_after_it():
    mats, hier, _ = R.scenario("jit-jit45")
    B = dev(np.column_stack([R.rhs(seed=s) for s in (7, 8, 9)]))
    H = hierarchy(mats[0], hier)

    def run_block(bc, graph):
        bc.use_columns(3)
        bc.levels[0].b[:, :3].copy_(B)
        for _ in range(2):
            if graph:
                bc.captured(2, 0.8).launch()
            else:
                bc.cycle(2, 0.8)
        return bc.levels[0].x.clone()

    vals = dev(mats[1].data)
    with torch.cuda.stream(H.stream):
        bc = BlockCycle(H, 3)
        first = run_block(bc, False), run_block(bc, True)
        H.rebuild_numeric(vals)
        old = run_block(bc, False), run_block(bc, True)
        new = run_block(BlockCycle(H, 3), False)
    torch.cuda.synchronize()
    assert torch.equal(first[0], first[1])
    assert torch.equal(old[0], new) and torch.equal(old[1], new)
    assert not torch.equal(old[0][:, :3], first[0][:, :3]) and not bool(old[0][:, 3].any())
    # column 0 against the hierarchy's own cycles on the same right-hand side, at the bound for cycles (other kernels)
    F = hierarchy(mats[1], hier)
    with torch.cuda.stream(F.stream):
        F.levels[0].b.copy_(B[:, 0].contiguous())
        F.cycle("Jacobi", 2, 0.8, x_is_zero=True)
        F.cycle("Jacobi", 2, 0.8)
        want = F.levels[0].x.clone()
    torch.cuda.synchronize()
    worst = R.within_cycle_bound(old[0][:, 0], want, float(np.linalg.norm(R.rhs(seed=7))))
    print("block column 0 against the single-vector cycle: %.3g of the bound for cycles" % worst)
    assert worst <= 1.0


def test_mass_and_operator_rebuilds_do_not_disturb_each_other():
    """The mass-like matrix of test_mass_matrix_coarsening_on_the_device (tests/test_solvers_gpu.py).  The coarse mass
    matrices are SciPy's products bit for bit, as there, whatever happened to the operator in between; the operator's state is
    that of a fresh hierarchy, whatever happened to the mass matrix."""
    import scipy.sparse as sp
    A = R.matrix("const")
    hier = list(R.transfers("const"))
    rng = np.random.default_rng(3)
    M1, M2 = (sp.csr_matrix((rng.random(A.nnz) + 0.1, A.indices.copy(), A.indptr.copy()), shape=A.shape) for _ in range(2))

    def assert_masses(H, Mx):
        want = Mx
        for l, Pm in enumerate(hier):
            want = sp.csr_matrix(sp.csr_matrix(Pm.T @ want) @ Pm)
            got = H.levels[l + 1].M.to_scipy()
            assert got.shape == want.shape and abs(got - want).max() == 0.0, l

    H = hierarchy(A, hier, mass=M1)
    assert_masses(H, M1)
    rebuild(H, R.matrix("var45"))
    assert_masses(H, M1)
    with torch.cuda.stream(H.stream):
        H.rebuild_mass_numeric(dev(M2.data))
    torch.cuda.synchronize()
    assert_masses(H, M2)
    assert H.generation == 1                                            # (counts the operator's rebuilds)
    R.assert_same_state(H, hierarchy(R.matrix("var45"), hier))
    rebuild(H, A)                                                       # the replay path of the operator's product maps
    assert_masses(H, M2)
    with torch.cuda.stream(H.stream):
        H.rebuild_mass_numeric(dev(M1.data))                            # ... and of the mass matrix's
    torch.cuda.synchronize()
    assert_masses(H, M1)
    R.assert_same_state(H, hierarchy(A, hier), same_kinds=False)        # (back on constant values: the formats stay)
    assert H.generation == 2


def test_a_wrong_number_of_values_raises_and_changes_nothing():
    mats, hier, _ = R.scenario("const-var45")
    cfg = R.CONFIGS["cheby-3"]
    H = hierarchy(mats[0], hier)
    prepare(H, cfg)
    b = dev(R.rhs())
    x1, x2, g = run(H, cfg, b)
    was = [lev.A.vals.clone() for lev in H.levels]
    for numel in (mats[0].nnz - 1, mats[0].nnz + 1, 0):
        with pytest.raises(ValueError):
            H.rebuild_numeric(torch.ones(numel, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    assert H.generation == 0 and len(H._graphs) == 1
    assert all(torch.equal(lev.A.vals, v) for lev, v in zip(H.levels, was))
    R.assert_same_state(H, H)
    y1, y2, g2 = run(H, cfg, b)
    assert g2 is g and torch.equal(y1, x1) and torch.equal(y2, x2)
