"""Cycles, captured graphs, preconditioners and solves on operators that are NOT numbered line by line on a grid (-m gpu).

Every other whole-cycle test of the suite runs on grid-ordered operators, where pack() hands every level a stencil, row-pattern,
DIA or SELL twin, Gauss-Seidel runs the wavefront kernel, the transfers fold into fused passes and the coarsest solve is the
grid-block solver.  A Morton- or randomly numbered operator takes another path on every level: packed CSR (int32 columns once a
512-row tile spans 65536 columns), the level-schedule executors of csr_gs_schedule (the ELL kernel, and behind it the chain
kernel, the one-workgroup kernel and a launch per set: gs_executor below), the two-launch Chebyshev step, separate transfer SpMVs, the dense or RCM-ordered coarse solver, and a refusal for Line.  The kernels have their own parity tests; here
they run together, against oracle.vcycle_ref.HoistedVCycle under the tolerance rule of tests/reorder.py, with the premises --
which twin, which executor, which solver -- asserted, so that a change of rule shows as a premise failure.

The set counts asserted below are those of the product's level schedule, which levels A + A^T (the reversed schedule is then the
exact backward sweep): the identity rows of the boundary wait for the interior rows that read them, so the fine levels have 511
sets of at most 514 rows (Morton 257^2) and 15 sets of at most 13536 (random 257^2, seed 5), where levelling A alone gives 510
sets / 1024 and 15 / 14040.  Either way the executor is the same.

Each test prints its largest deviation in units of the rule's atol before it asserts."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import chebyshev_ref as C                                          # noqa: E402
import reorder as RO                                               # noqa: E402
from block_cg_ref import pcg_ref                                   # noqa: E402
from krylov_ref import fgmres_ref                                  # noqa: E402
from learnmultigrid_amd import coarse as CS, ops, problems as P    # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy                 # noqa: E402
from learnmultigrid_amd.solvers import CG, GMRES, HierarchyMG     # noqa: E402
from oracle import kernels as K                                    # noqa: E402  (checker only)
from oracle.vcycle_ref import HoistedVCycle, RefMultigrid          # noqa: E402  (checker only)
from support import DEV, dev, galerkin9, nan_vec                   # noqa: E402

GRID_TWINS = ("patterns", "stencil", "prolong", "restrict", "dia")


def to_dev(t):
    return t.to(DEV)


def twins(M):
    """The names of the twins a matrix has, and the column mode of its packed or sliced-ELL twin."""
    names = tuple(name for name in GRID_TWINS + ("sell", "packed") if getattr(M, name) is not None)
    T = M.packed if M.packed is not None else M.sell
    return names + (None if T is None else int(T.colmode),)


def twin_table(H):
    return [tuple(None if M is None else twins(M) for M in (lev.A, lev.P, lev.R)) for lev in H.levels]


def tile_span(M, rows=512):
    """The widest column span max - min of a tile of `rows` rows: what decides uint16 or int32 columns in the packed CSR."""
    M = sp.csr_matrix(M)
    out = 0
    for r0 in range(0, M.shape[0], rows):
        c = M.indices[M.indptr[r0]:M.indptr[min(r0 + rows, M.shape[0])]]
        if c.size:
            out = max(out, int(c.max()) - int(c.min()))
    return out


def operators(kind, numbering, m=256):
    """(A, P, R, first Galerkin operator) of the reordered two-level problem on the host, canonical CSR."""
    Ap, Hp, _, _ = RO.reordered(kind, numbering, m, 2)
    R = K.as_csr(Hp[0].T.tocsr())
    return Ap, Hp[0], R, K.as_csr(sp.csr_matrix((R @ Ap) @ Hp[0]))


def packed(M):
    d = ops.DeviceCSR.from_scipy(M, DEV)
    d.pack()
    return d


def gs_executor(A, sched):
    """How csr_gs_schedule runs `sched` on A, by its own rules: "ell5" / "ell9" / ... (the one-workgroup ELL kernel on rows of
    at most 16 entries), "chain" (at most 4 rows a set: one wave, row after row), "one-workgroup" (sets of at most
    gs_single_max rows), "per-set" (one launch per set)."""
    n = int(sched.h_ptr[-1])
    ell = ops._gs_ell(A, sched)
    if ell is not None and ell[1] is not None:
        assert ell[2] is sched.d_rows and n > 4 * sched.nsets and sched.max_set <= ops.GS_ELL_MAX_SET
        return "ell%d" % ell[1]
    if n <= 4 * sched.nsets:
        assert ell is None
        return "chain"
    return "one-workgroup" if sched.max_set <= ops.tune_get("gs_single_max") else "per-set"


# the executor of every smoothed level that sweeps by a level schedule, by (kind, numbering, m): what the set counts of the
# product's schedule give (tests/test_reordered_cpu.py needs no GPU for them; the fine level of const-mixed runs the wavefront)
EXECUTORS = {("const", "morton", 64): ["ell5", "ell9"], ("const", "random", 64): ["ell5", "ell9"], ("const", "mixed", 64): ["ell9"],
             ("var", "morton", 64): ["ell5", "ell9"], ("var", "random", 64): ["ell5", "ell9"], ("var", "mixed", 64): ["ell5", "ell9"],
             ("learned", "morton", 64): ["ell5", "chain"], ("learned", "random", 64): ["ell5", "one-workgroup"],
             ("learned", "mixed", 64): ["ell5", "one-workgroup"], ("var", "random", 256): ["per-set", "ell9", "ell9"]}


def run(H, b, smoother, graph=False, cycles=RO.CYCLES, **kw):
    """(norms, iterate) of `cycles` cycles of RO.STEPS sweeps from zero, eager or replayed from the captured cycle."""
    g = None
    if graph:
        with torch.cuda.stream(H.stream):
            g = H.captured_cycle(smoother, RO.STEPS, RO.OMEGA, kw.get("gs_mode", "lexicographic"))
    return RO.hierarchy_history(H, b, cycles, smoother, RO.STEPS, RO.OMEGA, graph=g, to=to_dev, **kw)


def check_against_oracle(H, case, what=""):
    """Jacobi and forward Gauss-Seidel on H against RO.reference(*case, smoother): the rule on the history and the iterate, the
    replayed capture equal to the eager cycle bit for bit, check_smoothers() after the Gauss-Seidel runs."""
    bp = RO.reordered(*case)[2]
    for smoother in RO.SMOOTHERS:
        want, atols, xs = RO.reference(*case, smoother)
        got, x = run(H, bp, smoother)
        print("%s %s %s: device %.4f atol, iterate %.2e max|x|"
              % (what, case, smoother, RO.deviation(got, want, atols), np.abs(x - xs[-1]).max() / np.abs(xs[-1]).max()))
        RO.assert_history(got, want, atols, smoother)
        RO.assert_iterate(x, xs[-1], smoother)
        got2, x2 = run(H, bp, smoother, graph=True)
        assert np.array_equal(got2, got) and np.array_equal(x2, x), smoother
        if smoother == "GaussSeidel":
            H.check_smoothers()


# ---- premises: which twin a reordered operator gets ----------------------------------------------------------------------------
def test_random_257_gets_int32_columns_and_morton_keeps_uint16():
    Ar, Pr, Rr, Gr = operators("const", "random")
    assert (tile_span(Ar), tile_span(Pr), tile_span(Rr)) == (66045, 16639, 66047)
    want = {"A": 1, "P": 0, "R": 1, "G": 0}
    for name, M in zip("APRG", (Ar, Pr, Rr, Gr)):
        d = packed(M)
        assert twins(d) == ("packed", want[name]), (name, twins(d))
    Am, Pm, Rm, Gm = operators("const", "morton")
    assert max(tile_span(M) for M in (Am, Pm, Rm, Gm)) == 44728
    for name, M in zip("APRG", (Am, Pm, Rm, Gm)):
        d = packed(M)
        assert twins(d) == ("packed", 0), (name, twins(d))


@pytest.mark.parametrize("kind", ["const", "var", "learned"])
def test_mixed_hierarchy_keeps_its_fine_twin_and_folds_no_transfer(kind):
    """Fine level in grid order, coarse levels random: level 0 runs the fused passes, but its transfers map onto no grid --
    every availability check of a folded transfer says no, for the Jacobi and the Chebyshev passes and for the turnaround pass.
    (That the cycle then computes the right thing is test_cycles_match_the_oracle_... on the "mixed" cases.)"""
    case = (kind, "mixed", 64, 3)
    Ap, Hp, bp, _ = RO.reordered(*case)
    H = Hierarchy(Ap, Hp, DEV)
    l0, l1 = H.levels[0], H.levels[1]
    assert (l0.A.stencil is not None) if kind == "const" else (l0.A.dia is not None and l0.A.stencil is None)
    assert ops.stencil_smooth_available(l0.A) and ops.stencil_cheby_available(l0.A)
    for lev in H.levels[:-1]:
        for M in (lev.P, lev.R):
            assert M.prolong is None and M.restrict is None, twins(M)
        assert not ops.stencil_smooth_prolong_available(lev.A, lev.P)
        assert not ops.stencil_smooth_restrict_available(lev.A, lev.R)
        assert not ops.stencil_smooth_turnaround_available(lev.A, lev.P, lev.R)
        assert not ops.stencil_smooth_turnaround_selected(lev.A, lev.P, lev.R)
        assert not ops.stencil_cheby_prolong_available(lev.A, lev.P)
        assert not ops.stencil_cheby_restrict_available(lev.A, lev.R)
    assert l1.A.stencil is None and l1.A.dia is None, twins(l1.A)
    assert not ops.stencil_smooth_available(l1.A) and not ops.stencil_gs_available(l1.A)
    assert ops.stencil_gs_available(l0.A) == (kind == "const")


# ---- the three executors of csr_gs_schedule ---------------------------------------------------------------------------------------
def _gs_operator(name):
    if name == "random257":
        return operators("const", "random")[0]
    if name == "morton257":
        return operators("const", "morton")[0]
    if name == "learned_random33_25pt":
        return RO.hoisted("learned", "random", 64, 3).A[1]
    side, order = {"random129_9pt": (129, RO.random_order(129 * 129, 6)), "morton17_9pt": (17, RO.morton_order(17))}[name]
    G = galerkin9(side)
    return K.as_csr(G[order][:, order])


@pytest.mark.parametrize("name,nsets,widest,executor", [
    ("random257", 15, 13536, "per-set"),           # wider than GS_ELL_MAX_SET: one launch per set
    ("random129_9pt", 18, 1902, "ell9"),           # (seed 6; close to GS_ELL_MAX_SET: seeds 7 and 8 give 1882 and 1847)
    ("morton257", 511, 514, "ell5"),
    ("morton17_9pt", 94, 6, "chain"),              # 289 rows in 94 sets: the one-wave chain kernel
    ("learned_random33_25pt", 36, 48, "one-workgroup"),   # 25-entry rows: too long for the ELL copy
])
def test_every_level_schedule_executor_on_a_reordered_operator(name, nsets, widest, executor):
    """Forward and backward sweeps, 1 and 3 of them, bit for bit against the oracle's lexicographic sweep; a forward and a
    reversed schedule on the same matrix keep their own schedule-ordered patterns."""
    A = _gs_operator(name)
    dA = packed(A)
    n = A.shape[0]
    fwd = ops.build_gs_schedule(A, "lexicographic", DEV)
    bwd = fwd.reversed()
    assert (fwd.nsets, fwd.max_set) == (nsets, widest) == (bwd.nsets, bwd.max_set)
    assert ops.GS_ELL_MAX_SET == 2048
    for sched in (fwd, bwd):
        assert gs_executor(dA, sched) == executor
    rng = np.random.default_rng(5)
    x0, b = rng.standard_normal(n), rng.standard_normal(n)
    rows = {"f": np.arange(n, dtype=np.int32), "b": np.arange(n - 1, -1, -1, dtype=np.int32)}
    x, want = dev(x0), x0.copy()
    for sched, key, sweeps in ((fwd, "f", 1), (bwd, "b", 1), (fwd, "f", 3), (bwd, "b", 3)):      # (alternating: each keeps its own)
        ops.csr_gs_schedule(dA, x, dev(b), sched, sweeps)
        for _ in range(sweeps):
            K.gs_rows(A, want, b, rows[key])
        assert np.array_equal(x.cpu().numpy(), want), (key, sweeps)


# ---- kernel parity on the reordered operators -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["const", "learned"])
def test_sweeps_on_the_operators_of_random_257_are_the_oracles_bits(kind):
    rng = np.random.default_rng(257)
    for name, M in zip("APRG", operators(kind, "random")):
        d = packed(M)
        assert all(getattr(d, t) is None for t in GRID_TWINS), (name, twins(d))
        nr, nc = M.shape
        x, y0 = rng.standard_normal(nc), rng.standard_normal(nr)
        for alpha, beta in ((1.0, 0.0), (1.0, 1.0), (-0.5, 2.0)):
            y = dev(y0) if beta != 0.0 else nan_vec(nr)
            ops.csr_spmv(d, dev(x), y, alpha, beta)
            assert np.array_equal(y.cpu().numpy(), K.spmv(M, x, y0, alpha, beta)), (name, twins(d), alpha, beta)
        if nr != nc:
            continue
        r, out = nan_vec(nr), nan_vec(nr)
        part = torch.empty(ops.partials_count(nr), dtype=torch.float64, device=DEV)
        n2 = torch.zeros(1, dtype=torch.float64, device=DEV)
        ops.csr_residual_norm2(d, dev(x), dev(y0), r, part, n2)
        wr, wn2 = K.residual(M, x, y0)
        assert np.array_equal(r.cpu().numpy(), wr), (name, twins(d))
        assert abs(n2.item() - wn2) <= 1e-13 * wn2, (name, twins(d))
        ops.csr_jacobi(d, dev(x), dev(y0), 0.8, out)
        assert np.array_equal(out.cpu().numpy(), K.jacobi(M, x, y0, 0.8)), (name, twins(d))


# ---- cycles against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,numbering,m,levels", RO.CYCLE_CASES)
def test_cycles_match_the_oracle_and_their_captures_replay_bit_for_bit(kind, numbering, m, levels):
    case = (kind, numbering, m, levels)
    Ap, Hp, bp, _ = RO.reordered(*case)
    H = Hierarchy(Ap, Hp, DEV)
    print(twin_table(H))
    for lev in H.levels[(1 if numbering == "mixed" else 0):-1]:
        assert all(getattr(lev.A, t) is None for t in ("stencil", "dia")), twins(lev.A)
        assert not ops.stencil_smooth_available(lev.A) and not ops.stencil_gs_available(lev.A)
    for lev in H.levels[:-1]:
        assert lev.P.prolong is None and lev.R.restrict is None
    if m == 256:
        assert H.sizes == [66049, 16641, 4225, 1089] and H.coarse.kind == "dense"
        assert [twins(M) for M in (H.levels[0].A, H.levels[0].P, H.levels[0].R)] == [("packed", 1), ("packed", 0), ("packed", 1)]
    else:
        assert H.sizes == [4225, 1089, 289] and H.coarse.kind == "dense"
    check_against_oracle(H, case)
    execs = [gs_executor(lev.A, lev.gs_sched["lexicographic"]) for lev in H.levels[:-1] if "lexicographic" in lev.gs_sched]
    print("executors", execs)
    assert execs == EXECUTORS[kind, numbering, m]


@pytest.mark.parametrize("numbering", RO.NUMBERINGS)
def test_multicolour_gauss_seidel_is_deterministic_and_contracts(numbering):
    """There is no reference for the order of a greedy colouring: two hierarchies give identical bits, every cycle contracts,
    and the replayed capture is the eager cycle."""
    Ap, Hp, bp, _ = RO.reordered("var", numbering, 64, 3)
    runs = []
    for _ in range(2):
        H = Hierarchy(Ap, Hp, DEV)
        runs.append(run(H, bp, "GaussSeidel", gs_mode="multicolor"))
        H.check_smoothers()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    got, x = run(H, bp, "GaussSeidel", graph=True, gs_mode="multicolor")
    assert np.array_equal(got, runs[0][0]) and np.array_equal(x, runs[0][1])
    t = runs[0][0]
    print("multicolour %s: %s" % (numbering, t))
    # (the lexicographic sweep of the reference reaches 3e-6 of the start in these six cycles)
    assert np.all(t[1:] < t[:-1]) and t[-1] < 1e-3 * t[0], t


# ---- equivariance: the packed and two-launch paths against the fused grid passes -----------------------------------------------------
CHEBY = dict(cheby_lmax=2.2, cheby_ratio=4.0)
_grid_runs = {}


def _grid_run(kind, smoother):
    """The grid-order hierarchy's (norms, iterate) after 4 cycles, computed once per (kind, smoother) on the fused passes."""
    if (kind, smoother) not in _grid_runs:
        A, hier, rhs = RO.problem(kind, 64, 3)
        H = Hierarchy(A, list(hier), DEV)
        fused = (ops._cheby_kind if smoother == "Chebyshev" else ops._fused_kind)(H.levels[0].A)
        assert fused == ("tile" if kind == "const" else "dia"), fused
        _grid_runs[kind, smoother] = run(H, rhs, smoother, cycles=4, **(CHEBY if smoother == "Chebyshev" else {}))
    return _grid_runs[kind, smoother]


@pytest.mark.parametrize("smoother", ["Jacobi", "Chebyshev"])
@pytest.mark.parametrize("numbering", ["morton", "random"])
@pytest.mark.parametrize("kind", ["const", "var"])
def test_the_reordered_iterate_is_the_grid_iterate_renumbered(kind, numbering, smoother):
    """Jacobi and Chebyshev do not know the numbering (tests/test_reordered_cpu.py shows it for the reference): the packed
    sweeps, the two-launch Chebyshev step, the separate transfers and the dense coarse solve give, un-permuted, the iterate
    of the fused grid passes with the grid-block coarse solve."""
    A, hier, rhs = RO.problem(kind, 64, 3)
    Ap, Hp, bp, orders = RO.reordered(kind, numbering, 64, 3)
    kw = CHEBY if smoother == "Chebyshev" else {}
    want, x_grid = _grid_run(kind, smoother)
    H = Hierarchy(Ap, Hp, DEV)
    assert not ops.stencil_smooth_available(H.levels[0].A) and not ops.stencil_cheby_available(H.levels[0].A)
    got, x = run(H, bp, smoother, cycles=4, **kw)
    atols = np.full(5, RO.tolerances(A, x_grid, rhs))                    # (the largest iterate of the run: the solution grows)
    err = np.abs(RO.unpermute(x, orders[0]) - x_grid).max() / np.abs(x_grid).max()
    print("%s %s %s: history %.4f atol, iterate %.2e max|x|; %s" % (kind, numbering, smoother, RO.deviation(got, want, atols), err, got))
    RO.assert_iterate(RO.unpermute(x, orders[0]), x_grid)
    RO.assert_history(got[-1:], want[-1:], atols[-1:])
    assert np.all(got[2:] < 0.5 * got[1:-1]), got


def test_chebyshev_two_launch_cycle_matches_its_reference():
    """The Chebyshev cycle on a random numbering against tests/chebyshev_ref.ChebyCycle, eager and replayed."""
    Ap, Hp, bp, _ = RO.reordered("var", "random", 64, 3)
    ref = C.ChebyCycle.galerkin(Ap, Hp, lmax=[CHEBY["cheby_lmax"]] * 2, ratio=CHEBY["cheby_ratio"])
    want, atols, xs = RO.oracle_history(ref, Ap, bp, 4, degree=RO.STEPS)
    H = Hierarchy(Ap, Hp, DEV)
    got, x = run(H, bp, "Chebyshev", cycles=4, **CHEBY)
    print("chebyshev var random: device %.4f atol" % RO.deviation(got, want, atols))
    RO.assert_history(got, want, atols)
    RO.assert_iterate(x, xs[-1])
    with torch.cuda.stream(H.stream):
        g = H.captured_cycle("Chebyshev", RO.STEPS, 1.0, "lexicographic", **CHEBY)
    got2, x2 = RO.hierarchy_history(H, bp, 4, "Chebyshev", RO.STEPS, graph=g, to=to_dev)
    assert np.array_equal(got2, got) and np.array_equal(x2, x)


# ---- the coarse solver ------------------------------------------------------------------------------------------------------------
def test_a_morton_coarsest_level_of_4225_rows_dense_and_cyclic_reduction():
    case = ("var", "morton", 128, 2)
    Ap, Hp, bp, _ = RO.reordered(*case)
    H = Hierarchy(Ap, Hp, DEV, coarse_solver="auto")
    Ah = H.levels[-1].A.to_scipy()
    n, w = Ah.shape[0], CS.half_bandwidth(Ah)
    plan = CS.BandedBlockSolver.plan(n, w)
    # the not-banded branch: no grid, no banded plan within its byte limit, and small enough for the plain inverse
    assert n == 4225 and CS.GridBlockSolver.detect_grid(n, Ah) is None
    assert plan is None or 8 * (2 * plan[0] * plan[1] ** 2 + (n - plan[0] * plan[1]) ** 2) > CS.BANDED_MAX_BYTES, (w, plan)
    assert 8 * n * n <= CS.DENSE_PREFERRED_BYTES and H.coarse.kind == "dense"
    check_against_oracle(H, case, "auto")
    del H
    H = Hierarchy(Ap, Hp, DEV, coarse_solver="bcr")
    assert H.coarse.kind == "block-cyclic-reduction" and H.coarse.perm is not None            # (built on the RCM order)
    assert w > 4 * int(np.sqrt(n)) + 8
    check_against_oracle(H, case, "bcr")


# ---- rebuild_numeric ----------------------------------------------------------------------------------------------------------------
def test_rebuild_numeric_on_a_random_numbering_equals_a_fresh_hierarchy():
    A1p, Hp, bp, orders = RO.reordered("var", "random", 64, 3)
    A2 = P.variable_coeff_poisson_2d_structured(64, seed=45)[0]
    A2p, _, _ = RO.reorder(A2, [], bp, orders[:1])
    assert np.array_equal(A2p.indices, A1p.indices) and np.array_equal(A2p.indptr, A1p.indptr)
    H = Hierarchy(A1p, Hp, DEV)
    before = twin_table(H)
    run(H, bp, "GaussSeidel", cycles=1)                                  # (schedules and their patterns exist before the rebuild)
    H.rebuild_numeric(dev(A2p.data))
    fresh = Hierarchy(A2p, Hp, DEV)
    assert twin_table(H) == before == twin_table(fresh)
    for l, (a, f) in enumerate(zip(H.levels, fresh.levels)):
        assert torch.equal(a.A.vals, f.A.vals) and torch.equal(a.A.colidx, f.A.colidx) and torch.equal(a.A.rowptr, f.A.rowptr), l
    ref = HoistedVCycle(A2p, Hp)
    for smoother in RO.SMOOTHERS:
        want, atols, xs = RO.oracle_history(ref, A2p, bp, RO.CYCLES, smoother=smoother, steps=RO.STEPS, omega=RO.OMEGA)
        got, x = run(H, bp, smoother)
        print("rebuilt %s: device %.4f atol" % (smoother, RO.deviation(got, want, atols)))
        RO.assert_history(got, want, atols, smoother)
        RO.assert_iterate(x, xs[-1], smoother)
        got2, x2 = run(fresh, bp, smoother)
        assert np.array_equal(got2, got) and np.array_equal(x2, x), smoother
    H.check_smoothers()


# ---- the front ends ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smoother", RO.SMOOTHERS)
@pytest.mark.parametrize("numbering", ["morton", "random"])
def test_hierarchymg_solve_matches_the_reference_solver(numbering, smoother):
    case = ("var", numbering, 32, 3)
    Ap, Hp, bp, _ = RO.reordered(*case)
    kw = dict(levels=3, smoother=smoother, smooth_steps=RO.STEPS, max_iterations=RO.CYCLES + 1, error=1e-30, omega=RO.OMEGA)
    ref = RefMultigrid(Ap, bp.reshape(-1, 1).copy(), hierarchy=Hp)
    ref.solve(semantics="as_named", **kw)
    mg = HierarchyMG(Ap, bp.reshape(-1, 1).copy(), Hp)
    mg.solve(smoother_semantics="as_named", **kw)
    got, want = mg.get_track_res().ravel(), ref.track_res.ravel()
    _, atols, xs = RO.reference(*case, smoother)                          # (the iterates of the same cycles, for the rule's atol)
    assert got.shape == want.shape == (RO.CYCLES + 1,) and got[0] == want[0] == np.sqrt(Ap.shape[0])
    print("HierarchyMG %s %s: device %.4f atol" % (numbering, smoother, RO.deviation(got[1:], want[1:], atols[1:RO.CYCLES + 1])))
    RO.assert_history(got[1:], want[1:], atols[1:RO.CYCLES + 1])
    assert mg.level_dims == ref.level_dims == [1089, 289, 81]
    RO.assert_iterate(mg.get_solution(), ref.solution)
    mg2 = HierarchyMG(Ap, bp.reshape(-1, 1).copy(), Hp)
    mg2.solve(smoother_semantics="as_named", use_graph=True, **kw)
    assert np.array_equal(mg2.get_track_res(), mg.get_track_res()) and np.array_equal(mg2.get_solution(), mg.get_solution())


def _iterations_to(solver_cls, A, b, H, **kw):
    s = solver_cls(A, b.reshape(-1, 1).copy())
    s.solve(max_iterations=60, error=1e-9 * np.linalg.norm(b), preconditioner=H, **kw)
    assert s.get_residual() <= 1e-9 * np.linalg.norm(b)
    return s.get_iterations()


@pytest.mark.parametrize("solver", ["CG", "GMRES"])
def test_krylov_solvers_preconditioned_by_a_reordered_hierarchy(solver):
    """Six iterations against the NumPy recurrences (block_cg_ref.pcg_ref, krylov_ref.fgmres_ref) driven by the oracle's
    cycle; atol of entry j from the reference's iterate after j iterations.  Then to 1e-9: as many iterations as the
    grid-order run, give or take one."""
    case = ("sym", "random", 64, 3)
    A, hier, rhs = RO.problem(*case[:1], *case[2:])
    Ap, Hp, bp, _ = RO.reordered(*case)
    assert abs(Ap - Ap.T).max() <= 1e-12 * abs(Ap).max()
    ref = RO.hoisted(*case)

    def M(v):
        return ref.cycle(np.zeros(Ap.shape[0]), v, "Jacobi", RO.STEPS, RO.OMEGA)
    its = RO.CYCLES
    kw = dict(precond_smoother="Jacobi", precond_steps=RO.STEPS, precond_omega=RO.OMEGA)
    H = Hierarchy(Ap, Hp, DEV)
    if solver == "CG":
        want, Xs = pcg_ref(Ap, bp, M, its)
        s = CG(Ap, bp.reshape(-1, 1).copy())
        s.solve(max_iterations=its, error=0.0, preconditioner=H, **kw)
    else:
        runs = [fgmres_ref(Ap, bp, M, restart=30, max_iterations=j, error=0.0) for j in range(its + 1)]
        want, Xs = np.array(runs[-1][1]), [r[0] for r in runs]
        s = GMRES(Ap, bp.reshape(-1, 1).copy())
        s.solve(max_iterations=its, error=0.0, restart=30, preconditioner=H, **kw)
    got = s.get_track_res().ravel()
    atols = np.array([RO.tolerances(Ap, x, bp) for x in Xs])
    print("%s sym random: device %.4f atol; %s" % (solver, RO.deviation(got, want, atols), got))
    RO.assert_history(got, want, atols)
    RO.assert_iterate(s.get_solution(), Xs[-1])
    cls = CG if solver == "CG" else GMRES
    n_perm = _iterations_to(cls, Ap, bp, H, **kw)
    n_grid = _iterations_to(cls, A, rhs, Hierarchy(A, list(hier), DEV), **kw)
    print("%s iterations: reordered %d, grid order %d" % (solver, n_perm, n_grid))
    assert abs(n_perm - n_grid) <= 1 and n_perm < 40


def test_solve_many_columns_match_the_oracles_single_solves():
    """Three columns on the learned random hierarchy.  The block path runs sliced-ELL twins of its own and the single-vector
    path the packed CSR, so the two are not bit-equal with each other: each column is held to the oracle's solve of it.
    (Measured: 0.002 atol on the problem's own column; 0.56 atol on the two random columns, at entry 0, where x = 0 and the
    figure is the order in which ||b|| = 65.6 is summed -- 9e-16 relative, the rule's relative term.)"""
    case = ("learned", "random", 64, 3)
    Ap, Hp, bp, _ = RO.reordered(*case)
    B = np.column_stack([bp, np.random.default_rng(5).standard_normal((Ap.shape[0], 2))])
    mg = HierarchyMG(Ap, B[:, :1].copy(), Hp)
    X, track = mg.solve_many(B, levels=3, smooth_steps=RO.STEPS, max_iterations=RO.CYCLES + 1, error=0.0, omega=RO.OMEGA)
    assert track.shape == (RO.CYCLES + 1, 3) and X.shape == B.shape
    ref = RO.hoisted(*case)
    for j in range(3):
        want, atols, xs = (RO.reference(*case, "Jacobi") if j == 0 else
                           RO.oracle_history(ref, Ap, B[:, j], RO.CYCLES, smoother="Jacobi", steps=RO.STEPS, omega=RO.OMEGA))
        worst = int(np.argmax(np.abs(track[:, j] - want) / atols))
        print("solve_many column %d: device %.4f atol (entry %d: %.16e, oracle %.16e)"
              % (j, RO.deviation(track[:, j], want, atols), worst, track[worst, j], want[worst]))
        RO.assert_history(track[:, j], want, atols, "column %d" % j)
        # (X is the iterate after the cycle that follows the last recorded norm)
        RO.assert_iterate(X[:, j], ref.cycle(xs[-1], B[:, j], "Jacobi", RO.STEPS, RO.OMEGA), "column %d" % j)


# ---- Line: the refusal --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numbering,level", [("morton", 0), ("random", 0), ("mixed", 1)])
def test_line_is_refused_with_the_level_named_and_the_hierarchy_stays_usable(numbering, level):
    case = ("var", numbering, 64, 3)
    Ap, Hp, bp, _ = RO.reordered(*case)
    H = Hierarchy(Ap, Hp, DEV)
    with pytest.raises(ValueError, match=r"cannot run on level %d \(\d+ rows\): no 3x3 grid geometry" % level):
        H.prepare_smoother("Line")
    with pytest.raises(ValueError, match="level %d " % level):
        with torch.cuda.stream(H.stream):
            H.captured_cycle("Line", 1, 1.0, "lexicographic")
    want, atols, xs = RO.reference(*case, "Jacobi")
    got, x = run(H, bp, "Jacobi")
    print("after the refusal %s: device %.4f atol" % (numbering, RO.deviation(got, want, atols)))
    RO.assert_history(got, want, atols)
    RO.assert_iterate(x, xs[-1])
