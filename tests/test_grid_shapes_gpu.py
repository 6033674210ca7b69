"""The fused smoothing passes off the square grid (-m gpu): the register pass (csrc/stencil_fused.hip), the LDS-tiled pass
(csrc/stencil_tile.hip) and the variable-coefficient pass (csrc/dia_tile.hip) against the CPU oracle's separate Jacobi
sweeps and residual applied to the CSR matrix itself -- the oracle knows nothing of lines -- bit for bit, on operators
whose boundary rows keep their couplings (tests/grid_ops.py):

  * operators with an entry ACROSS THE END OF A LINE of the stride their twin chose: x-periodic 5- and 9-point operators,
    and 7-point operators on a Wg x Hg grid that (Wg + 1) divides, which the twins read as the sheared stencil of stride
    Wg + 1.  Row W - 1 then reaches row 0 through slot 2 at tile coordinates (line -1, column W), row n - W reaches row
    n - 1 through slot 6 at (line `lines`, column -1): valid rows of the matrix outside the lines 0 .. lines - 1;
  * plain rectangles: wide and short, narrow and tall, widths and line counts around the multiples of a tile's inner part;
  * a ragged last line (leading principal blocks);
  * the grid transfers folded into the passes on a 97 x 65 grid, and a short 3-level cycle on it.

Every case first asserts which twin, stride and slot mask the operator got, so that it cannot silently stop exercising
its path; where a pass does not take an operator the refusal is asserted and the separate sweeps' bits are checked."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import chebyshev_ref as C                                            # noqa: E402  (checker only)
import fused_checks as FC                                            # noqa: E402
import grid_ops as G                                                 # noqa: E402
from fused_checks import (check_smoothing, cheby_knobs as knobs, first_diff, jacobi_wants, nested_pair,   # noqa: E402
                          register_pass)
from learnmultigrid_amd import ops                                   # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy                   # noqa: E402
from oracle import kernels as K                                      # noqa: E402  (checker only)
from oracle import vcycle_ref as V                                   # noqa: E402
from support import DEV, dev, nan_vec                                # noqa: E402


def expected_view(Wg, n, slots, periodic_x):
    """(line stride, union mask) the twins must choose, from their rule (twins.line_stride, DiaTwin.from_csr): of the strides
    that make every offset a 3x3 slot, the first of (largest offset, - 1, + 1) that divides n.  A 7-point operator
    {+-1, +-Wg, +-(Wg + 1)} also reads as the other orientation of stride Wg + 1, which comes first where it divides n; the
    wrap-around links of an x-periodic operator are the slots 2 and 6 of stride Wg."""
    if slots == 0x1BB and not periodic_x and n % (Wg + 1) == 0:
        return Wg + 1, 0x0FE
    return Wg, (slots | 0x44) if periodic_x else slots


def check_separate(tag, dA, x0, b, wants):
    """The path a refused operator takes: one launch per sweep, then the residual launch."""
    n = dA.shape[0]
    x, y, db, r = dev(x0), nan_vec(n), dev(b), nan_vec(n)
    for S in (1, 2, 3):
        ops.csr_jacobi(dA, x, db, 0.8, y)
        x, y = y, x
        got = x.cpu().numpy()
        assert np.array_equal(got, wants[0.8, False, S][0]), (tag, S, "separate sweeps", first_diff(got, wants[0.8, False, S][0]))
    ops.csr_residual_norm2(dA, x, db, r, None, None)
    assert np.array_equal(r.cpu().numpy(), wants[0.8, False, 3][1]), (tag, "separate residual")


def run_operator(tag, Wg, Hg, slots, values, periodic_x=False, rows=None, line_end=False, seed=1):
    """All the passes an operator takes against the oracle; the twin, its stride and mask, and whether an entry crosses a
    line end are asserted first."""
    A = G.grid_op(Wg, Hg, slots, values, periodic_x, rows, seed)
    n = A.shape[0]
    assert n >= max(ops.TILED_MIN_ROWS, ops.DiaTwin.MIN_ROWS)
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack()
    W, umask = expected_view(Wg, n, slots, periodic_x)
    if values == "row":
        assert dA.stencil is None and dA.dia is not None, tag
        T, kind = dA.dia, "dia"
    else:
        assert dA.stencil is not None and dA.dia is None, tag
        T = dA.stencil
        kind = "tile" if umask in (0x0BA, 0x1FF) else None          # the stencil passes are built for 5 and 9 points
    assert (T.W, T.umask) == (W, umask), (tag, T.W, hex(T.umask))
    assert (G.line_end_coupling(A, T.W).size > 0) == line_end, tag
    assert ops._fused_kind(dA) == kind and ops._cheby_kind(dA) == kind, tag
    rng = np.random.default_rng(n + seed)
    x0, b = rng.standard_normal(n), rng.standard_normal(n)
    wants = jacobi_wants(A, x0, b)
    lmax = C.gershgorin(A)
    check_separate(tag, dA, x0, b, wants)
    if kind == "dia":
        for rr in (32, 64):
            with knobs(dia_rows=rr):
                check_smoothing((tag, "dia_rows", rr), dA, x0, b, wants)
                FC.check_plain(A, dA, x0, b, lmax)
        return
    L = ops._lib.lib()
    if kind == "tile":
        for rr in (16, 32):
            with knobs(tile_rows=rr, tile_rows_big=rr):
                check_smoothing((tag, "tile_rows", rr), dA, x0, b, wants)
                FC.check_plain(A, dA, x0, b, lmax)
    else:
        # neither stencil pass is built for this slot set: the hierarchy runs the separate sweeps (checked above), and a
        # direct call answers with an error instead of a result
        assert not L.lmg_stencil_smooth_tiled_supported(umask) and not L.lmg_stencil_smooth_supported(umask)
        assert not ops.stencil_smooth_available(dA) and not ops.stencil_cheby_available(dA)
        with pytest.raises(ops.LmgError):
            ops.stencil_smooth(dA, dev(x0), dev(b), 0.8, 1, nan_vec(n))
        return
    assert L.lmg_stencil_smooth_supported(umask)
    for seg in (0, 5):
        with register_pass(seg):
            assert ops._fused_kind(dA) is None
            check_smoothing((tag, "register pass, seg_lines", seg), dA, x0, b, wants)


# ---- entries across the end of a line -----------------------------------------------------------------------------------------
LINE_END = {
    # x-periodic 5-point: {-W, -W + 1, -1, 0, 1, W - 1, W}
    "periodic5_70x60": dict(Wg=70, Hg=60, slots=0x0BA, periodic_x=True, line_end=True),
    # x-periodic 9-point (the links along the line wrap, the diagonal ones do not): the one slot set with a line-end entry
    # that the stencil passes are built for
    "periodic9_70x60": dict(Wg=70, Hg=60, slots=0x1FF, periodic_x=True, line_end=True),
    # 7-point on 64 x 65: 65 divides n and comes first, the sheared stride; grid node (1, 0) is row W - 1 and reaches
    # node (0, 0) through slot 2
    "sheared7_64x65": dict(Wg=64, Hg=65, slots=0x1BB, line_end=True),
    # the mirror: 66 does not divide n, the grid's own stride is chosen -- no entry crosses a line end
    "plain7_65x64": dict(Wg=65, Hg=64, slots=0x1BB, line_end=False),
    # the other orientation on 63 x 66: its second stride, 62, comes after 63 in the candidates and 63 always divides n, so a
    # whole rectangle of this orientation never shears ...
    "plain7b_63x66": dict(Wg=63, Hg=66, slots=0x0FE, line_end=False),
    # narrow and tall, 8 | 7 * 800: sheared, a line end every 8 rows (eight grid lines inside one 64-column tile)
    "sheared7_7x800": dict(Wg=7, Hg=800, slots=0x1BB, line_end=True),
}


@pytest.mark.parametrize("values", ["const", "row"])
@pytest.mark.parametrize("name", sorted(LINE_END))
def test_line_end_coupling(name, values):
    run_operator((name, values), values=values, **LINE_END[name])


def test_sheared_the_other_way_with_a_ragged_last_line():
    """... but its leading block of 62 * 67 rows does: 63 no longer divides, 62 does.  The sheared entries are the slots 0
    and 8 of stride 62, which leave the matrix at both ends instead of re-entering it, yet the lines still matter: row
    n - W sits in column 0 and reads row n - W - 1 through slot 3, i.e. the tile element (line lines - 1, column -1), whose
    own neighbour below is (line `lines`, column -1) = row n - 1."""
    Wg, Hg, rows = 63, 66, 62 * 67
    A = G.grid_op(Wg, Hg, 0x0FE, "row", rows=rows, seed=2)
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack()
    assert dA.dia is not None and (dA.dia.W, dA.dia.umask) == (62, 0x1BB) and G.line_end_coupling(A, 62).size > 0
    rng = np.random.default_rng(rows)
    x0, b = rng.standard_normal(rows), rng.standard_normal(rows)
    wants = jacobi_wants(A, x0, b)
    for rr in (32, 64):
        with knobs(dia_rows=rr):
            check_smoothing(("sheared7b", rr), dA, x0, b, wants)
            FC.check_plain(A, dA, x0, b, C.gershgorin(A))


# ---- plain rectangles -----------------------------------------------------------------------------------------------------------
# A tile stores its inner 64 - 2 H columns and RR - 2 H lines, H = 0 .. 4 the halo of the pass, RR = 16, 32 or 64 lines.
#   1400 x 4            wide and short: fewer lines than any tile's inner part, 22 - 25 tiles across
#   5 x 900, 7 x 800    narrow and tall: 12 / 9 grid lines inside one 64-column tile; from 600 lines on the tiled pass takes
#                       its tile height from tile_rows_big
#   55, 56, 57 wide     one below, at and one above 64 - 2 * 4; 113 = 2 * 56 + 1: a third tile for one column
#   75, 74, 73 lines    around 72 = 3 * (32 - 2 * 4) = 9 * (16 - 2 * 4) = 6 * (16 - 2 * 2) and 74 = 37 * (16 - 2 * 7)... : one
#                       to three lines into the last tile line for the halos 2 .. 4 of both tile heights; 37 = 36 + 1
RECTANGLES = [(1400, 4), (5, 900), (7, 800), (55, 75), (56, 74), (57, 73), (113, 37)]
# (7 x 800 with the 0x1BB orientation shears: it is in LINE_END; here it takes the other one)


def rect_cases():
    out = []
    for k, (Wg, Hg) in enumerate(RECTANGLES):
        for slots in (0x0BA, 0x1BB, 0x1FF):
            if slots == 0x1BB and (Wg * Hg) % (Wg + 1) == 0:
                slots = 0x0FE
            # 5 and 9 points on every shape; the 7-point operators, which only the DIA pass runs fused, on every other one
            for values in ("const", "row"):
                if slots in (0x1BB, 0x0FE) and values == "const" and k % 2:
                    continue
                out.append(pytest.param(Wg, Hg, slots, values, id="%dx%d-%03x-%s" % (Wg, Hg, slots, values)))
    return out


@pytest.mark.parametrize("Wg,Hg,slots,values", rect_cases())
def test_rectangles(Wg, Hg, slots, values):
    run_operator(("rect", Wg, Hg, hex(slots), values), Wg, Hg, slots, values, line_end=False, seed=3)


# ---- a ragged last line -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", ["const", "row"])
@pytest.mark.parametrize("slots", [0x0BA, 0x1FF])
@pytest.mark.parametrize("short", [1, 13, 40])
def test_ragged_last_line(short, slots, values):
    """n = 61 * 70 - short rows: the last line ends `short` columns early, in the middle of the tiles and strips that hold
    it.  All three passes take such an operator (their front ends ask for no whole number of lines).  61 lines: one more
    than 2 * (32 - 2), 5 * (16 - 4) and 64 - 4 -- the short line is a tile line of its own for some halo of every tile
    height, so a line count rounded down loses it."""
    run_operator(("ragged", short, hex(slots), values), 70, 61, slots, values, rows=61 * 70 - short, line_end=False, seed=4)


# ---- the transfers folded into the passes, on a rectangle ------------------------------------------------------------------
@pytest.mark.parametrize("slots", [0x0BA, 0x1FF])
def test_transfer_passes_on_a_rectangle(slots):
    """Fine 97 x 65, coarse 49 x 33: R (b - A J^S x) and J^S (x + P e) of the tiled and the register family against the
    oracle.  pack() alone finds no grid map for a transfer between rectangles (it tries square grids and 1-D): the
    transfers stay unfused then, which is asserted; told the two line lengths, as the distributed levels tell it, it
    builds the window twins and the passes take them."""
    Wf, Hf = 97, 65
    A = G.grid_op(Wf, Hf, slots, "const", seed=5)
    Pm, Rm = nested_pair(Wf, Hf)
    n, nc = A.shape[0], Pm.shape[1]
    assert (n, nc) == (97 * 65, 49 * 33)
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack()
    assert dA.stencil is not None and (dA.stencil.W, dA.stencil.umask) == (Wf, slots) and ops._fused_kind(dA) == "tile"
    rng = np.random.default_rng(97)
    x0, b, e = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(nc)
    # as the hierarchy packs them: no window twins, no folded transfers; the separate launches give the oracle's bits
    dP, dR = ops.DeviceCSR.from_scipy(Pm, DEV), ops.DeviceCSR.from_scipy(Rm, DEV)
    dP.pack()
    dR.pack()
    assert dP.prolong is None and dR.restrict is None
    assert not ops.stencil_smooth_prolong_available(dA, dP) and not ops.stencil_smooth_restrict_available(dA, dR)
    assert not ops.stencil_cheby_prolong_available(dA, dP) and not ops.stencil_cheby_restrict_available(dA, dR)
    xe, bc = dev(x0), nan_vec(nc)
    ops.csr_spmv(dP, dev(e), xe, 1.0, 1.0)
    assert np.array_equal(xe.cpu().numpy(), K.spmv(Pm, e, x0.copy(), 1.0, 1.0))
    r0 = K.residual(A, x0, b)[0]
    ops.csr_spmv(dR, dev(r0), bc)
    assert np.array_equal(bc.cpu().numpy(), K.spmv(Rm, r0))
    # with the line lengths: the twins, and the passes of both families
    dP, dR = ops.DeviceCSR.from_scipy(Pm, DEV), ops.DeviceCSR.from_scipy(Rm, DEV)
    dP.pack(line_strides=(Wf, 49))
    dR.pack(line_strides=(Wf, 49))
    TP, TR = dP.prolong, dR.restrict
    assert TP is not None and (TP.W, TP.Wc, TP.nc) == (Wf, 49, nc)
    assert TR is not None and (TR.W, TR.Wc, TR.nc, TR.n) == (Wf, 49, nc, n)
    assert ops.stencil_smooth_prolong_available(dA, dP) and ops.stencil_smooth_restrict_available(dA, dR)
    for layout in FC.LAYOUTS:
        for hx in (1, 0):
            with FC.tile_knobs(tile_hot_transfers=hx, **layout):
                FC.check_pre(A, Rm, dA, dR, x0, b)
                FC.check_post(A, Pm, dA, dP, x0, b, e)
    lmax = C.gershgorin(A)
    for rr in (16, 32):
        with knobs(tile_rows=rr, tile_rows_big=rr):
            FC.check_transfers(A, Pm, Rm, dA, dP, dR, x0, b, e, lmax)
    for seg in (0, 5):
        with register_pass(seg):
            assert ops._fused_kind(dA) is None
            FC.check_pre(A, Rm, dA, dR, x0, b)
            FC.check_post(A, Pm, dA, dP, x0, b, e)


def test_tiled_transfer_passes_on_an_operator_with_line_end_coupling():
    """The tiled passes find the coarse window of an element from its own line and column wherever it sits in the tile, so
    they fold the transfers of an x-periodic operator too (71 x 61 -> 36 x 31); the register pass takes the coarse column
    from the lane number, which is wrong beyond a line end: it refuses such an operator's transfers."""
    Wf, Hf = 71, 61
    A = G.grid_op(Wf, Hf, 0x1FF, "const", periodic_x=True, seed=6)
    Pm, Rm = nested_pair(Wf, Hf)
    n, nc = A.shape[0], Pm.shape[1]
    dA, dP, dR = (ops.DeviceCSR.from_scipy(M, DEV) for M in (A, Pm, Rm))
    dA.pack()
    dP.pack(line_strides=(Wf, 36))
    dR.pack(line_strides=(Wf, 36))
    assert dA.stencil is not None and (dA.stencil.W, dA.stencil.umask) == (Wf, 0x1FF)
    assert G.line_end_coupling(A, Wf).size > 0 and dP.prolong is not None and dR.restrict is not None
    assert ops.stencil_smooth_prolong_available(dA, dP) and ops.stencil_smooth_restrict_available(dA, dR)
    rng = np.random.default_rng(71)
    x0, b, e = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(nc)
    for layout in FC.LAYOUTS:
        for hx in (1, 0):
            with FC.tile_knobs(tile_hot_transfers=hx, **layout):
                FC.check_pre(A, Rm, dA, dR, x0, b)
                FC.check_post(A, Pm, dA, dP, x0, b, e)
    assert dA.stencil.line_end_coupling
    with register_pass(0):
        with pytest.raises(ops.LmgError):
            ops.stencil_smooth(dA, dev(x0), dev(b), 0.8, 1, nan_vec(n), None, prolong=(dP, dev(e)))
        with pytest.raises(ops.LmgError):
            ops.stencil_smooth(dA, dev(x0), dev(b), 0.8, 1, nan_vec(n), None, restrict=(dR, nan_vec(nc)))
    min_tr = ops.FUSED_TRANSFER_MIN_ROWS
    try:
        ops.FUSED_TRANSFER_MIN_ROWS = 0
        assert not ops._prolong_available(dA, dP, "reg") and not ops._restrict_available(dA, dR, "reg")
        assert not dA.stencil.gs_ok
    finally:
        ops.FUSED_TRANSFER_MIN_ROWS = min_tr


# ---- one short cycle ----------------------------------------------------------------------------------------------------------------
def test_three_level_cycles_on_a_rectangle_with_live_boundary_rows():
    """97 x 65 -> 49 x 33 -> 25 x 17, 3 cycles: the Jacobi history against the oracle's cycle and the Chebyshev history
    against its CPU twin at the suite's rtol = 1e-10; the same bits with the fused passes off.  (The off-diagonal entries
    are made negative: an M-matrix, so that the cycles converge and the comparison is one of converging histories.)"""
    A = G.grid_op(97, 65, 0x0BA, "const", seed=7)
    d = A.diagonal()
    A = K.as_csr(sp.csr_matrix(sp.diags(d) - abs(A - sp.diags(d))))
    hier = [nested_pair(97, 65)[0], nested_pair(49, 33)[0]]
    n = A.shape[0]
    rhs = np.random.default_rng(65).standard_normal(n)
    H = Hierarchy(A, hier, DEV)
    assert [lev.n for lev in H.levels] == [97 * 65, 49 * 33, 25 * 17]
    assert ops._fused_kind(H.levels[0].A) == "tile" and H.levels[0].A.stencil.W == 97

    def jacobi_history():
        with torch.cuda.stream(H.stream):
            H.levels[0].b.copy_(dev(rhs))
            ops.zero(H.levels[0].x)
            hist = [H.residual_norm()]
            for _ in range(3):
                H.cycle("Jacobi", 3, 0.8)
                hist.append(H.residual_norm())
            return hist, H.levels[0].x.cpu().numpy().copy()

    h1, x1 = jacobi_history()
    ref = V.HoistedVCycle(A, [sp.csr_matrix(q) for q in hier])
    x = np.zeros(n)
    want = [np.linalg.norm(rhs - A @ x)]
    for _ in range(3):
        x = ref.cycle(x, rhs, "Jacobi", 3, 0.8)
        want.append(np.linalg.norm(rhs - A @ x))
    print("Jacobi history", h1, "oracle", want)
    np.testing.assert_allclose(h1, want, rtol=1e-10, atol=1e-14 * max(want))
    c1, xc1 = FC.cheby_histories(H, rhs, 3, 3)
    cw, _, _ = FC.cheby_twin_history(A, rhs, hier, 3, 3, H=H)
    print("Chebyshev history", c1, "twin", cw)
    np.testing.assert_allclose(c1, cw, rtol=1e-10, atol=1e-14 * max(cw))
    try:
        ops.set_fused_enabled(False)
        assert not ops.stencil_smooth_available(H.levels[0].A)
        h0, x0 = jacobi_history()
        c0, xc0 = FC.cheby_histories(H, rhs, 3, 3)
    finally:
        ops.set_fused_enabled(True)
    assert h1 == h0 and np.array_equal(x1, x0)
    assert np.array_equal(c1, c0) and np.array_equal(xc1, xc0)
