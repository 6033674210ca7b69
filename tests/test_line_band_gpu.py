"""Line relaxation with banded line systems on the GPU (-m gpu): lmg_line_factor_banded and lmg_line_solve_banded
(csrc/line.hip) against the NumPy twin (tests/line_band_ref.py) bit for bit, their flags and argument checks, that a 3x3
hierarchy keeps its bits under line_band=3, whole cycles on a hierarchy of learned-type transfers (levels with half-bandwidth
1 / 2 / 3) against the twin's cycles, graph replay, and CG / GMRES preconditioned with such a cycle.

Shapes.  19 x 13 and 70 x 67: lines of 19, 13, 70 and 67 elements go through the solve kernels in blocks of 32 (direction
x) / 16 (direction y), then 8, then single elements -- x: 19 = 2 * 8 + 3 and 70 = 2 * 32 + 6; y: 13 = 8 + 5 and
67 = 4 * 16 + 3 --, the factorisation in blocks of 4; 70 and 67 systems are two workgroups, 13 and 19 one partly filled
wave; lines of 13 are shorter than one long block.  75 x 59 runs all three stages in one line, the chain handed from a long
block to a short one: 75 = 2 * 32 + 8 + 3 in x, 59 = 3 * 16 + 8 + 3 in y."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import line_band_ref as LB                                          # noqa: E402  (checker only)
from block_cg_ref import first_pass, pcg_ref                        # noqa: E402  (checker only)
from krylov_ref import fgmres_ref                                   # noqa: E402  (checker only)
from learnmultigrid_amd import _lib, ops, problems as P             # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy                  # noqa: E402
from oracle import kernels as K                                     # noqa: E402  (checker only)
from support import DEV, dev                                        # noqa: E402

SENTINEL, TAIL = -7.25, 96


def _headed(values=None, n=None):
    """A tensor of n + TAIL doubles whose head holds `values` (NaN without) and whose tail holds SENTINEL."""
    n = len(values) if values is not None else n
    t = torch.full((n + TAIL,), SENTINEL, dtype=torch.float64, device=DEV)
    t[:n] = dev(values) if values is not None else float("nan")
    return t


def _tail_intact(t, n):
    return bool((t[n:] == SENTINEL).all())


# ---- 1. the two entry points against the twin, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("Wg,Hg", [(19, 13), (70, 67), (75, 59)])
def test_factor_and_solve_equal_the_twin_bit_for_bit(Wg, Hg, p):
    A = LB.window_operator(Wg, Hg, p, seed=100 * p + Wg)
    n = A.shape[0]
    assert np.unique(A.data).size == A.nnz and np.diff(A.indptr).max() == (2 * p + 1) ** 2
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(Wg * 1000 + Hg + p)
    x0, r0 = rng.standard_normal(n), rng.standard_normal(n)
    for d in "xy":
        want_fac, want_flags = LB.factor(A, Wg, d, p)
        fac = _headed(n=(2 * p + 1) * n)
        flags = torch.zeros(1, dtype=torch.int32, device=DEV)
        assert L.lmg_line_factor_banded(n, Wg, ops.LINE_DIRS[d], p, dA.rowptr.data_ptr(), dA.colidx.data_ptr(),
                                        dA.vals.data_ptr(), fac.data_ptr(), flags.data_ptr(), st) == 0
        assert int(flags.item()) == want_flags == 0
        got = fac[:(2 * p + 1) * n].cpu().numpy().reshape(2 * p + 1, n)
        for k in range(2 * p + 1):
            assert np.array_equal(got[k], want_fac[k]), (d, "plane", k, np.flatnonzero(got[k] != want_fac[k])[:8])
        assert _tail_intact(fac, (2 * p + 1) * n)
        # the ops wrapper gives the same block
        f2, fl2 = ops.line_factor_banded_flags(dA, Wg, d, p)
        assert fl2 == 0 and torch.equal(f2, fac[:(2 * p + 1) * n])
        for first, step in ((0, 1), (0, 2), (1, 2), (2, 3)):
            for omega in (1.0, 0.8):
                x, r = _headed(x0), _headed(r0)
                assert L.lmg_line_solve_banded(n, Wg, ops.LINE_DIRS[d], p, first, step, fac.data_ptr(), r.data_ptr(), omega,
                                               x.data_ptr(), st) == 0
                wx, wr = LB.solve(want_fac, Wg, d, p, first, step, r0, omega, x0)
                gx, gr = x[:n].cpu().numpy(), r[:n].cpu().numpy()
                assert np.array_equal(gx, wx), (d, first, step, omega, np.flatnonzero(gx != wx)[:8])
                assert np.array_equal(gr, wr), (d, first, step, omega, np.flatnonzero(gr != wr)[:8])
                assert _tail_intact(x, n) and _tail_intact(r, n)
                keep = np.ones(LB.by_system(x0, Wg, d).shape, dtype=bool)
                keep[first::step] = False
                assert np.array_equal(LB.by_system(gx, Wg, d)[keep], LB.by_system(x0, Wg, d)[keep])
                assert np.array_equal(LB.by_system(gr, Wg, d)[keep], LB.by_system(r0, Wg, d)[keep])
                assert keep.any() == (step > 1) and not np.array_equal(gx, x0)
        assert _tail_intact(fac, (2 * p + 1) * n)


def test_lines_shorter_than_the_band_and_the_ops_wrapper():
    """Lines of 2 and 3 elements under half-bandwidth 3 (with so short a line an x-offset of 3 is the next line's node, so the
    operators keep the entries of their own lines only); the solve through ops.line_solve_banded."""
    import scipy.sparse as sp
    for Wg, Hg, d in ((3, 9, "x"), (2, 9, "x"), (9, 3, "y"), (9, 2, "y")):
        coo = LB.window_operator(Wg, Hg, 1, seed=Wg).tocoo()
        off = coo.col.astype(np.int64) - coo.row
        own = (coo.row // Wg == coo.col // Wg) if d == "x" else (off % Wg == 0)
        A = K.as_csr(sp.csr_matrix((coo.data[own], (coo.row[own], coo.col[own])), shape=coo.shape))
        n = A.shape[0]
        dA = ops.DeviceCSR.from_scipy(A, DEV)
        rng = np.random.default_rng(n)
        x0, r0 = rng.standard_normal(n), rng.standard_normal(n)
        want_fac, want_flags = LB.factor(A, Wg, d, 3)
        fac = ops.line_factor_banded(dA, Wg, d, 3)
        assert want_flags == 0 and np.array_equal(fac.cpu().numpy(), want_fac.reshape(-1))
        x, r = dev(x0), dev(r0)
        ops.line_solve_banded(Wg, d, 3, 0, 1, fac, r, 0.8, x)
        wx, wr = LB.solve(want_fac, Wg, d, 3, 0, 1, r0, 0.8, x0)
        assert np.array_equal(x.cpu().numpy(), wx) and np.array_equal(r.cpu().numpy(), wr)
        # what the short lines solve is the system itself
        Ad = A.toarray()
        e = (wx - x0) / 0.8
        assert np.linalg.norm(Ad @ e - r0) <= 1e-12 * np.linalg.norm(r0)


# ---- 2. flags and errors ----------------------------------------------------------------------------------------------------------
def test_flags():
    import scipy.sparse as sp
    Wg, Hg = 19, 13
    A = LB.window_operator(Wg, Hg, 2, seed=7)
    C = A.tolil()
    C[3 * Wg + 1, 3 * Wg - 1] = 0.25                               # offset -2 from column 1 of line 3: leaves the line
    C = K.as_csr(sp.csr_matrix(C))
    dC = ops.DeviceCSR.from_scipy(C, DEV)
    assert ops.line_factor_banded_flags(dC, Wg, "x", 2)[1] == ops.LINE_COUPLED == LB.factor(C, Wg, "x", 2)[1]
    assert ops.line_factor_banded_flags(dC, Wg, "y", 2)[1] == 0 == LB.factor(C, Wg, "y", 2)[1]
    with pytest.raises(ValueError, match="couples two x-lines"):
        ops.line_factor_banded(dC, Wg, "x", 2)
    S = A.tolil()
    i = 5 * Wg
    S[i, i] = S[i, i + 1] = S[i + 1, i] = S[i + 1, i + 1] = 1.0    # a singular leading block of x-line 5
    S = K.as_csr(sp.csr_matrix(S))
    dS = ops.DeviceCSR.from_scipy(S, DEV)
    for p in (2, 3):
        assert ops.line_factor_banded_flags(dS, Wg, "x", p)[1] == ops.LINE_PIVOT == LB.factor(S, Wg, "x", p)[1]
        assert ops.line_factor_banded_flags(dS, Wg, "y", p)[1] == 0 == LB.factor(S, Wg, "y", p)[1]
    with pytest.raises(ValueError, match="pivot"):
        ops.line_factor_banded(dS, Wg, "x", 2)


def test_entry_points_check_their_arguments():
    """Every bad call answers LMG_ERR_ARG (-1) before anything is launched (the buffers keep their NaNs)."""
    W, Hg, p = 9, 7, 2
    A = LB.window_operator(W, Hg, p, seed=3)
    n = A.shape[0]
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    nan = lambda m: torch.full((m,), np.nan, dtype=torch.float64, device=DEV)
    fac, r, x = nan(7 * n), nan(n), nan(n)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    q = lambda t: t.data_ptr()
    good_f = [n, W, 0, p, q(dA.rowptr), q(dA.colidx), q(dA.vals), q(fac), q(flags), st]
    for at in (4, 5, 6, 7, 8):                                        # NULL pointers
        bad = list(good_f)
        bad[at] = None
        assert L.lmg_line_factor_banded(*bad) == -1, at
    for at, v in ((3, 1), (3, 4), (3, 0), (3, -2), (2, 2), (2, -1), (1, 0), (1, 8), (0, -1), (7, q(dA.vals))):
        bad = list(good_f)                                            # band, dir, stride, n % stride, n < 0, fac aliases vals
        bad[at] = v
        assert L.lmg_line_factor_banded(*bad) == -1, (at, v)
    good_s = [n, W, 1, p, 0, 1, q(fac), q(r), 1.0, q(x), st]
    for at in (6, 7, 9):
        bad = list(good_s)
        bad[at] = None
        assert L.lmg_line_solve_banded(*bad) == -1, at
    for at, v in ((3, 1), (3, 4), (5, 0), (5, -2), (4, -1), (2, 2), (2, -1), (1, 0), (1, 8), (0, -1)):
        bad = list(good_s)
        bad[at] = v
        assert L.lmg_line_solve_banded(*bad) == -1, (at, v)
    for at, v in ((7, q(x)), (7, q(fac) + 8 * 2 * n), (9, q(fac)), (9, q(fac) + 8 * (4 * n + 5))):   # r = x; r, x inside fac
        bad = list(good_s)
        bad[at] = v
        assert L.lmg_line_solve_banded(*bad) == -1, (at, v)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (fac, r, x)) and int(flags.item()) == 0
    for bad_band in (1, 4, True):
        with pytest.raises(ValueError, match="band"):
            ops.line_factor_banded(dA, W, "x", bad_band)
    with pytest.raises(ValueError):
        ops.line_factor_banded(dA, W, "z", 2)
    with pytest.raises(ValueError):
        ops.line_factor_banded(dA, 8, "x", 2)
    with pytest.raises(ValueError):
        ops.line_solve_banded(W, "x", 2, 0, 1, nan(5 * n - 1), r, 1.0, x)


def test_torch_ops_equal_the_ctypes_path():
    ops.register_torch_ops()
    Wg, Hg, p = 19, 13, 3
    A = LB.window_operator(Wg, Hg, p, seed=9)
    n = A.shape[0]
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    rng = np.random.default_rng(6)
    x0, r0 = rng.standard_normal(n), rng.standard_normal(n)
    for d in "xy":
        fac, flags = ops.line_factor_banded_flags(dA, Wg, d, p)
        f2, fl2 = torch.ops.lmg.line_factor_banded(dA.rowptr, dA.colidx, dA.vals, Wg, d, p)
        assert fl2 == flags == 0 and torch.equal(fac, f2)
        x1, r1, x2, r2 = dev(x0), dev(r0), dev(x0), dev(r0)
        ops.line_solve_banded(Wg, d, p, 1, 2, fac, r1, 0.8, x1)
        torch.ops.lmg.line_solve_banded(Wg, d, p, 1, 2, f2, r2, 0.8, x2)
        assert torch.equal(x1, x2) and torch.equal(r1, r2) and not torch.equal(x1, dev(x0))


# ---- 3. a 3x3 hierarchy keeps its bits -----------------------------------------------------------------------------------------------
def _histories(H, rhs, cycles, line_dir, shape="V", graph=False, **kw):
    fine = H.levels[0]
    with torch.cuda.stream(H.stream):
        H.prepare_smoother("Line", line_dir=line_dir, line_order="zebra", **kw)
        fine.b.copy_(dev(rhs.ravel()))
        ops.zero(fine.x)
        g = H.captured_cycle("Line", 1, 1.0, "lexicographic", shape=shape) if graph else None
        norms = [H.residual_norm()]
        for _ in range(cycles):
            if g is not None:
                g.launch()
            else:
                H.cycle("Line", 1, 1.0, shape=shape)
            norms.append(H.residual_norm())
        x = fine.x.cpu().numpy().copy()
    return np.array(norms), x


def test_a_five_point_hierarchy_keeps_its_bits_under_line_band_3():
    A, rhs = P.anisotropic_poisson_2d_structured(64, 1e-3, 1.0)
    hier = P.geometric_hierarchy_2d(65, 4)
    h0, x0 = _histories(Hierarchy(A, hier, DEV), rhs, 4, "xy")
    H = Hierarchy(A, hier, DEV)
    h3, x3 = _histories(H, rhs, 4, "xy", line_band=3)
    assert np.array_equal(h0, h3) and np.array_equal(x0, x3)
    assert [lev.line_band for lev in H.levels[:-1]] == [{"x": 1, "y": 1}] * 3 and H.line_key() == ("xy", "zebra", 3)


# ---- 4. cycles on a hierarchy of learned-type transfers ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def learned():
    """The 65^2 stretched problem (a_x = 1e-3 a_y), learned_like transfers 65 -> 33 -> 17 -> 9, a random right-hand side."""
    A, _ = P.anisotropic_poisson_2d_structured(64, 1e-3, 1.0)
    A = K.as_csr(A)
    rhs = np.random.default_rng(11).standard_normal(A.shape[0])
    hier = LB.transfers("learned_like")
    return A, rhs, hier, Hierarchy(A, hier, DEV)


def _twin_of(H, line_dir):
    """The twin on H's own level operators, the coarsest level solved by H's own direct solver."""
    last = H.levels[-1]

    def coarse(rc):
        with torch.cuda.stream(H.stream):
            last.b.copy_(dev(rc))
            H.coarse_solve()
            return last.x.cpu().numpy().copy()

    return LB.LineBandCycle([l.A.to_scipy() for l in H.levels], [l.P.to_scipy() for l in H.levels[:-1]],
                            [l.R.to_scipy() for l in H.levels[:-1]], coarse, [1, 2, 3], line_dir=line_dir)


@pytest.mark.parametrize("line_dir", ["y", "xy"])
def test_cycle_histories_match_the_twin_and_graph_replay_matches_eager(learned, line_dir):
    A, rhs, hier, H = learned
    for shape, cycles in (("V", 5), ("W", 3)):
        got, x = _histories(H, rhs, cycles, line_dir, shape, line_band=3)
        assert [lev.line["W"] for lev in H.levels[:-1]] == [65, 33, 17]
        assert [lev.line_band["y"] for lev in H.levels[:-1]] == [1, 2, 3]
        want, _ = LB.history(_twin_of(H, line_dir), A, rhs, cycles, steps=1, shape=shape)
        rel = np.abs(got - want) / want
        print("%s %s: history rel. diff max %.3e, per cycle %s" % (line_dir, shape, rel.max(), np.round(got[1:] / got[:-1], 4)))
        assert np.all(rel <= 1e-10), (line_dir, shape, rel)
        gg, xg = _histories(H, rhs, cycles, line_dir, shape, graph=True, line_band=3)
        assert np.array_equal(gg, got) and np.array_equal(xg, x), (line_dir, shape, "graph replay vs eager")


def test_graph_key_and_device_offsets(learned):
    A, rhs, hier, H = learned
    with torch.cuda.stream(H.stream):
        g1 = H.captured_cycle("Line", 1, 1.0, "lexicographic", line_dir="y", line_band=3)
        g2 = H.captured_cycle("Line", 1, 1.0, "lexicographic")
        g3 = H.captured_cycle("Line", 1, 1.0, "lexicographic", line_dir="xy")
        for l in (0, 1, 2):
            M = H.levels[l].A.to_scipy().tocoo()
            assert np.array_equal(H._device_offsets(l), np.unique(M.col.astype(np.int64) - M.row))
    assert g1 is g2 and g3 is not g1 and H.line_key() == ("xy", "zebra", 3)
    fresh = Hierarchy(A, hier, DEV)
    with pytest.raises(ValueError, match=r"level 1 \(1089 rows\): no 3x3 grid geometry"):
        fresh.prepare_smoother("Line")
    with pytest.raises(ValueError, match=r"level 2 \(289 rows\): no 5x5 grid geometry"):
        fresh.prepare_smoother("Line", line_band=2)


def test_a_refused_band_keeps_the_captured_cycle_valid(learned):
    """What a solve without the keyword does to a shared hierarchy: line_band None becomes 1 there, the 25-point level refuses
    it, and the hierarchy keeps band 3 with the factors the captured cycle points at -- also after the allocator has let go
    of everything it could and handed out new blocks."""
    A, rhs, hier, _ = learned
    H = Hierarchy(A, hier, DEV)
    eager, xe = _histories(H, rhs, 4, "y", line_band=3)
    with torch.cuda.stream(H.stream):
        g = H.captured_cycle("Line", 1, 1.0, "lexicographic")
        ptrs = [lev.line["y"].data_ptr() if torch.is_tensor(lev.line["y"]) else tuple(t.data_ptr() for t in lev.line["y"])
                for lev in H.levels[:-1]]
        with pytest.raises(ValueError, match=r"level 1 \(1089 rows\): no 3x3 grid geometry"):
            H.prepare_smoother("Line", line_dir="y", line_band=1)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        junk = [torch.full((n,), np.nan, dtype=torch.float64, device=DEV) for n in (4225, 3 * 4225, 5 * 1089, 7 * 289)]
        assert H.line_key() == ("y", "zebra", 3)
        assert H.captured_cycle("Line", 1, 1.0, "lexicographic", line_dir="y", line_band=3) is g
        assert ptrs == [lev.line["y"].data_ptr() if torch.is_tensor(lev.line["y"]) else tuple(t.data_ptr() for t in lev.line["y"])
                        for lev in H.levels[:-1]]
    replay, xr = _histories(H, rhs, 4, "y", graph=True, line_band=3)
    assert np.array_equal(replay, eager) and np.array_equal(xr, xe) and len(junk) == 4


def test_f_cycle_through_the_solver_front_end(learned):
    from learnmultigrid_amd.solvers import HierarchyMG
    A, rhs, hier, _ = learned
    mg = HierarchyMG(A, rhs.reshape(-1, 1).copy(), hier)
    u = mg.f_cycle(mg.matrix, np.zeros((A.shape[0], 1)), rhs.reshape(-1, 1), "Line", 1, 1e-8, 4, first_call=True,
                   smoother_semantics="as_named", line_dir="y", line_band=3)
    ref = LB.LineBandCycle.galerkin(A, hier, bands=[1, 2, 3], line_dir="y")
    w = ref.cycle(np.zeros(A.shape[0]), rhs, steps=1, shape="F")
    np.testing.assert_allclose(u.ravel(), w, rtol=0, atol=1e-10 * np.abs(w).max())
    mg2 = HierarchyMG(A, rhs.reshape(-1, 1).copy(), hier)
    mg2.solve(levels=4, smoother="Line", smoother_semantics="as_named", smooth_steps=1, max_iterations=12,
              error=1e-8 * np.linalg.norm(rhs), line_dir="y", line_band=3, use_graph=True)
    assert mg2.get_track_res()[-1, 0] <= 1e-8 * np.linalg.norm(rhs) and mg2.get_iterations() <= 11


# ---- 5. Krylov solvers preconditioned with the cycle -----------------------------------------------------------------------------
def test_mg_pcg_with_the_banded_line_cycle(learned):
    from learnmultigrid_amd.solvers import CG
    A = LB.symmetrised(learned[0])
    rhs, hier = learned[1], learned[2]
    H = Hierarchy(A, hier, DEV)
    error = 1e-8 * np.linalg.norm(rhs)
    cg = CG(A, rhs.reshape(-1, 1).copy())
    cg.solve(max_iterations=40, error=error, preconditioner=H, precond_smoother="Line", precond_steps=1, precond_omega=1.0,
             precond_line_band=3)
    got = cg.get_track_res().ravel()
    twin = _twin_of(H, "xy")
    M = lambda v: twin.cycle(np.zeros(A.shape[0]), v, steps=1, shape="V")
    want, _ = pcg_ref(A, rhs, M, cg.get_iterations() + 2)
    its = first_pass(np.asarray(want).reshape(-1, 1), error)[0]
    print("MG-PCG, Line(line_band=3): %d iterations (twin %d), history rel. diff max %.3e"
          % (cg.get_iterations(), its, np.max(np.abs(got - want[:got.size]) / want[:got.size])))
    assert cg.get_iterations() == its and got[-1] <= error
    np.testing.assert_allclose(got, np.asarray(want)[:got.size], rtol=1e-8, atol=0)


def test_fgmres_with_the_banded_line_cycle(learned):
    """The unsymmetric operator as it comes.  The solve stops at 1e-5 |b|: the last entry of a GMRES history is a recomputed
    norm |b - A x|, which carries an absolute rounding error of about eps |b| = 1.4e-14 here, so a relative 1e-8 can be
    asked of entries above 1.4e-6 only (measured when stopping at 1e-8 |b|: five entries within 1e-12, the last one,
    3.0e-8, off by 1.7e-14 = 5.7e-7 relative); the last entry of this solve is about 1e-4."""
    from learnmultigrid_amd.solvers import GMRES
    A, rhs, hier, H = learned
    error = 1e-5 * np.linalg.norm(rhs)
    g = GMRES(A, rhs.reshape(-1, 1).copy())
    g.solve(max_iterations=40, error=error, restart=20, preconditioner=H, precond_smoother="Line", precond_steps=1,
            precond_omega=1.0, precond_line_band=3)
    got = g.get_track_res().ravel()
    twin = _twin_of(H, "xy")
    M = lambda v: twin.cycle(np.zeros(A.shape[0]), v, steps=1, shape="V")
    _, want, its = fgmres_ref(A, rhs, M, restart=20, max_iterations=40, error=error)
    want = np.asarray(want).ravel()
    print("FGMRES, Line(line_band=3): %d iterations (twin %d), history rel. diff max %.3e"
          % (g.get_iterations(), its, np.max(np.abs(got - want) / want) if got.size == want.size else np.nan))
    assert g.get_iterations() == its and got[-1] <= error
    np.testing.assert_allclose(got, want, rtol=1e-8, atol=0)
