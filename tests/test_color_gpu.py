"""The "multicolor_device" Gauss-Seidel ordering on an MI355X (-m gpu): ops.color_device, ops.build_gs_schedule_device and
csrc/color.hip against the plain-Python twin of their rules (tests/color_ref.py) -- every integer equal --, the sweep on the
colour-ordered sliced-ELL twin against the per-set CSR executor and the twin's sequential walk, bit for bit, and whole solves
against a host statement of the same cycle.

Each whole-solve test prints its largest deviation from the host history, in units of the bound, before it asserts."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import amg_cases as C                                              # noqa: E402
import color_ref as K                                              # noqa: E402
import sa_cases as SC                                              # noqa: E402
from color_cases import CASES, case_matrices, coloring, complete, star      # noqa: E402
from learnmultigrid_amd import _lib, amg, ops                      # noqa: E402
from learnmultigrid_amd.solvers import CG, GMRES, ClassicalAMG, GaussSeidel, SmoothedAggregationAMG      # noqa: E402
from line_band_ref import symmetrised                              # noqa: E402
from support import DEV, dev                                       # noqa: E402

RTOL, FLOOR = 1e-10, 1e-14                                          # the project's standing bound for cycles (tests/test_amg_gpu.py)


def device_csr(A):
    return ops.DeviceCSR.from_scipy(sp.csr_matrix(A, dtype=np.float64), DEV, canonical=False)


# ---- the colouring and the schedule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_colours_rounds_and_schedule_are_the_twins(name):
    A = case_matrices()[name]
    want, nc, rounds = coloring(name)
    dA = device_csr(A)
    got, got_nc, got_rounds = ops.color_device(dA)
    assert (got_nc, got_rounds) == (nc, rounds)
    assert np.array_equal(got.cpu().numpy(), want)
    sched = ops.build_gs_schedule_device(dA)
    rows, ptr = K.schedule(want, nc)
    assert sched.kind == "multicolor_device" and sched.nsets == nc and not sched.backward
    assert np.array_equal(sched.d_rows.cpu().numpy(), rows) and np.array_equal(sched.h_ptr, ptr)
    back = sched.reversed()
    brows, bptr = K.reversed_schedule(rows, ptr)
    assert back.twin is sched.twin and back.backward and back.d_rows.is_cuda
    assert np.array_equal(back.d_rows.cpu().numpy(), brows) and np.array_equal(back.h_ptr, bptr)
    # the twin: every colour on a slice boundary, padded with rows -1
    T = sched.twin
    assert np.array_equal(T.h_color_slice, np.concatenate([[0], np.cumsum((np.diff(ptr) + 63) // 64)]))
    trow = T.trow.cpu().numpy()[:64 * T.nslices]
    for c in range(nc):
        part = trow[64 * T.h_color_slice[c]:64 * T.h_color_slice[c + 1]]
        k = ptr[c + 1] - ptr[c]
        assert np.array_equal(part[:k], rows[ptr[c]:ptr[c + 1]]) and np.all(part[k:] == -1)


def test_more_than_64_colours_are_refused_with_the_node():
    with pytest.raises(K.Refused) as want:
        K.color(complete(65))
    with pytest.raises(_lib.LmgError, match="node %d" % want.value.node):
        ops.color_device(device_csr(complete(65)))
    with pytest.raises(_lib.LmgError):
        ops.build_gs_schedule_device(device_csr(complete(65)))


# ---- the sweep ---------------------------------------------------------------------------------------------------------------
def broken_diagonals():
    """jittered 9 x 9 with the diagonal of row 30 removed and the diagonal of row 40 stored as 0.0: both rows stay as they are."""
    from learnmultigrid_amd import problems as P
    A = sp.csr_matrix(P.jittered_poisson_2d(8)[0], dtype=np.float64)
    A.sort_indices()
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    data = A.data.copy()
    data[(rows == 40) & (A.indices == 40)] = 0.0
    keep = ~((rows == 30) & (A.indices == 30))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    return sp.csr_matrix((data[keep], A.indices[keep], indptr), shape=A.shape)      # (the explicit 0.0 stays a stored entry)


@functools.lru_cache(maxsize=None)
def sweep_matrices():
    return {"level1": case_matrices()["level1"], "jittered32": case_matrices()["jittered32"],
            "broken_diagonals": broken_diagonals(), "star65": sp.csr_matrix(star(65), dtype=np.float64)}


@pytest.mark.parametrize("name", ["level1", "jittered32", "broken_diagonals", "star65"])
def test_sweep_is_the_csr_executors_and_the_twins_bits(name):
    A = sweep_matrices()[name]
    n = A.shape[0]
    dA = device_csr(A)
    sched = ops.build_gs_schedule_device(dA)
    col, nc, _ = K.color(A)
    rows, ptr = K.schedule(col, nc)
    assert np.array_equal(sched.d_rows.cpu().numpy(), rows)
    if name == "star65":
        assert 65 in np.diff(ptr)                                   # one full slice plus one lane
    if name == "broken_diagonals":
        assert 30 not in A.indices[A.indptr[30]:A.indptr[31]]
        assert A.data[A.indptr[40]:A.indptr[41]][list(A.indices[A.indptr[40]:A.indptr[41]]).index(40)] == 0.0
    rng = np.random.default_rng(11)
    x0, b = rng.standard_normal(n), rng.standard_normal(n)
    db = dev(b)
    for backward in (False, True):
        s = sched.reversed() if backward else sched
        order, optr = K.reversed_schedule(rows, ptr) if backward else (rows, ptr)
        plain = ops.GSSchedule("multicolor", order, optr, DEV)     # the same row list through the per-set CSR executor
        for sweeps in (1, 3):
            x1, x2, x3 = dev(x0.copy()), dev(x0.copy()), dev(x0.copy())
            ops.csr_gs_schedule(dA, x1, db, s, sweeps)
            ops.csr_gs_schedule(dA, x2, db, s, sweeps)
            ops.csr_gs_schedule(dA, x3, db, plain, sweeps)
            want = K.sweep(A, x0.copy(), b, order, sweeps)
            got = x1.cpu().numpy()
            what = "%s backward=%s sweeps=%d" % (name, backward, sweeps)
            assert torch.equal(x1, x2), what                        # two runs: equal bits
            assert torch.equal(x1, x3), what
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), what
            if name == "broken_diagonals":
                assert got[30] == x0[30] and got[40] == x0[40]


def test_gauss_seidel_solver_takes_the_mode():
    A, b = C.problems()["jittered"]
    b = b.ravel()
    col, nc, _ = coloring("jittered32")
    rows, _ptr = K.schedule(col, nc)
    for sweep, order in (("forward", [rows]), ("backward", [rows[::-1]]), ("symmetric", [rows, rows[::-1]])):
        gs = GaussSeidel(A, b.reshape(-1, 1).copy())
        gs.solve(max_iterations=4, error=0.0, gs_mode="multicolor_device", sweep=sweep)
        x = np.zeros(A.shape[0])
        want = []
        for _ in range(4):
            want.append(float(np.linalg.norm(b - A @ x)))
            for o in order:
                K.sweep(A, x, b, o)
        got = gs.get_track_res().ravel()
        assert np.all(np.abs(got - np.array(want)) <= RTOL * np.array(want)), sweep


# ---- whole solves ------------------------------------------------------------------------------------------------------------
def deviation(got, want, largest):
    """The largest |got - want| in units of the bound of tests/test_amg_gpu.py: 1e-10 relative with a floor of 1e-14 of
    `largest` = ||b||, the residual the run starts from."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / (RTOL * np.abs(want) + FLOOR * largest)))


def host_cycle(H, pair, steps=2):
    """The host statement of the cycle of the device hierarchy H: its operators and transfers pulled to the host, SciPy
    products, the twin's sequential sweep on the device's own schedules, a direct solve on the last level."""
    As = [lev.A.to_scipy() for lev in H.levels]
    Ps = [lev.P.to_scipy() for lev in H.levels[:-1]]
    scheds = []
    for l, lev in enumerate(H.levels[:-1]):
        s = H.gs_schedule(l, "multicolor_device")
        scheds.append((s.d_rows.cpu().numpy(), s.h_ptr))
        col, nc, _ = K.color(As[l])                                 # ... which are the twin's
        assert np.array_equal(scheds[-1][0], K.schedule(col, nc)[0])
    return K.VCycle(As, Ps, scheds, steps=steps, gs_sweep=pair)


SOLVE = dict(smoother="GaussSeidel", smooth_steps=2, smoother_semantics="as_named", gs_mode="multicolor_device")


def solver_for(kind):
    A, b = C.problems()["jittered"]
    if kind == "classical":
        return ClassicalAMG(A, b.reshape(-1, 1).copy(), **C.AMG_KW), A, b
    return SmoothedAggregationAMG(A, b.reshape(-1, 1).copy(), **dict(SC.SA_KW, theta=SC.THETA["jittered"])), A, b


@pytest.mark.parametrize("gs_sweep", ["forward", "symmetric", ("forward", "backward")], ids=["forward", "symmetric", "pair"])
@pytest.mark.parametrize("kind", ["classical", "sa"])
def test_whole_solves_match_the_host_statement(kind, gs_sweep):
    """V(2,2) to 1e-8 ||b||, at most the cap of the hierarchy's own tests (30 cycles classical, 60 smoothed aggregation)."""
    mg, A, b = solver_for(kind)
    cap = C.CAP if kind == "classical" else SC.CAP
    nb = np.linalg.norm(b)
    mg.solve(max_iterations=cap + 1, error=C.TARGET * nb, gs_sweep=gs_sweep, **SOLVE)
    got = mg.get_track_res().ravel()
    H = mg._hier
    assert all(lev.host_pattern is None for lev in H.levels)
    pair = (gs_sweep, gs_sweep) if isinstance(gs_sweep, str) else gs_sweep
    want = host_cycle(H, pair).history(b, cap, C.TARGET)
    m = min(got.size, len(want))
    print("%s %s: %d cycles (host %s), deviation %.3f of the bound"
          % (kind, gs_sweep, got.size - 1, C.cycles_needed(want), deviation(got[1:m], want[1:m], want[0])))
    assert C.cycles_needed(want) is not None and got.size - 1 == C.cycles_needed(want) <= cap and got[-1] <= C.TARGET * nb
    assert deviation(got[1:], want[1:], want[0]) <= 1.0
    # the captured cycle: the same history
    mg2, _, _ = solver_for(kind)
    mg2.solve(max_iterations=cap + 1, error=C.TARGET * nb, gs_sweep=gs_sweep, use_graph=True, **SOLVE)
    got2 = mg2.get_track_res().ravel()
    assert got2.size == got.size and deviation(got2[1:], want[1:], want[0]) <= 1.0
    assert all(lev.host_pattern is None for lev in mg2._hier.levels)


@functools.lru_cache(maxsize=None)
def symmetric_problem():
    A, b = C.problems()["jittered"]
    return symmetrised(A), b


def test_cg_with_the_symmetric_multicolour_cycle():
    A, b = symmetric_problem()
    nb = np.linalg.norm(b)
    H = amg.classical_hierarchy(A, DEV, **C.AMG_KW)
    kw = dict(preconditioner=H, precond_steps=2, precond_smoother="GaussSeidel", precond_gs_mode="multicolor_device")
    cg = CG(A, b.reshape(-1, 1).copy())
    cg.solve(max_iterations=C.CAP, error=C.TARGET * nb, **kw)
    print("CG: %d iterations" % cg.get_iterations())
    assert cg.get_residual() <= C.TARGET * nb and cg.get_iterations() <= C.CAP
    assert all(lev.host_pattern is None for lev in H.levels)
    g = GMRES(A, b.reshape(-1, 1).copy())
    g.solve(max_iterations=C.CAP, error=C.TARGET * nb, restart=10, **kw)
    assert g.get_residual() <= C.TARGET * nb
    with pytest.raises(ValueError, match="precond_gs_mode"):
        cg.solve(precond_gs_mode="nonsense", preconditioner=H)
    # M = one cycle from a zero iterate is a symmetric operator
    rng = np.random.default_rng(2024)
    u, v = rng.random(A.shape[0]), rng.random(A.shape[0])

    def M(w):
        with torch.cuda.stream(H.stream):
            H.levels[0].b.copy_(dev(w))
            H.cycle("GaussSeidel", 2, 1.0, "multicolor_device", x_is_zero=True, gs_sweep=("forward", "backward"))
            return H.levels[0].x.cpu().numpy().copy()

    Mu, Mv = M(u), M(v)
    diff = abs(float(np.dot(u, Mv)) - float(np.dot(Mu, v)))
    print("<u, Mv> - <Mu, v> = %.3e, bound %.3e" % (diff, 1e-12 * np.linalg.norm(u) * np.linalg.norm(Mv)))
    assert diff <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(Mv)


def test_a_cycle_after_rebuild_numeric_is_a_fresh_hierarchys():
    A, b = C.problems()["jittered"]
    A, b = sp.csr_matrix(A), b.ravel()
    H = amg.classical_hierarchy(A, DEV, **C.AMG_KW)
    rng = np.random.default_rng(5)
    # the same pattern, other values: the transfers stay, every coarse operator and every twin follows
    scale = 1.0 + 0.5 * rng.random(A.shape[0])
    D = sp.diags(np.sqrt(scale))
    A2 = sp.csr_matrix(D @ A @ D)
    A2.sort_indices()
    assert np.array_equal(A2.indices, A.indices) and np.array_equal(A2.indptr, A.indptr)

    def one_cycle(G):
        with torch.cuda.stream(G.stream):
            G.levels[0].b.copy_(dev(b))
            G.cycle("GaussSeidel", 2, 1.0, "multicolor_device", x_is_zero=True, gs_sweep=("forward", "backward"))
            return G.levels[0].x.clone()

    stale = one_cycle(H)                                            # (builds the schedules and twins on the old values)
    H.rebuild_numeric(dev(A2.data))
    got = one_cycle(H)
    # a fresh hierarchy on the new values with the same transfers
    Ps = [lev.P for lev in H.levels[:-1]]
    from learnmultigrid_amd.hierarchy import Hierarchy
    F = Hierarchy(device_csr(A2), Ps, DEV)
    want = one_cycle(F)
    assert torch.equal(got, want)
    assert not torch.equal(got, stale)
    assert all(lev.host_pattern is None for lev in H.levels)
