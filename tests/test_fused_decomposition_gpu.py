"""The work decomposition of the register-fused pass (csrc/stencil_fused.hip: launch4, decode_item) against the CPU
oracle's separate Jacobi sweeps and residual on the CSR matrix, bit for bit (-m gpu).

launch4 cuts the grid into boundary-strip items, edge segments and middle segments from fused_want_waves,
fused_want_waves_rest3, fused_floor_halos, fused_balance, fused_slow_pct, the segment-length keys and their line range;
fused_fast decides whether a wave may run the fast body.  The parity tests so far set fused_seg_lines only.  Here every one
of those keys is moved, on the 5- and the 9-point operator of tests/grid_ops.py (live boundary rows) on grids of W = 385
columns -- four strips, two boundary and two interior, for every halo width -- and few enough lines that every item count
is small.  The tiled pass is off, so these levels run the register pass.

Every output starts as NaN (the checkers of test_grid_shapes_gpu.py and test_tile_passes_gpu.py do that): a line that no
item owns shows as NaN, not as a stale value."""
import contextlib
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import fused_checks as FC                                            # noqa: E402
import grid_ops as G                                                 # noqa: E402
import sweep_variants as SV                                          # noqa: E402
from learnmultigrid_amd import ops                                   # noqa: E402

DEV = SV.DEV
W, LINES = 385, 97
SLOTS = [0x0BA, 0x1FF]
IDS = ["5pt", "9pt"]


@functools.lru_cache(maxsize=None)
def problem(slots, lines):
    """(A, x0, b, the oracle's J^S x and residuals) on the W x lines grid."""
    A = G.grid_op(W, lines, slots, "const", seed=11)
    n = A.shape[0]
    rng = np.random.default_rng(n + slots)
    x0, b = rng.standard_normal(n), rng.standard_normal(n)
    return A, x0, b, FC.jacobi_wants(A, x0, b)


@functools.lru_cache(maxsize=None)
def transfers():
    """P from the 193 x 49 grid to the 385 x 97 grid, its transpose, and a coarse vector."""
    Pm, Rm = FC.nested_pair(W, LINES)
    assert Pm.shape == (W * LINES, 193 * 49)
    return Pm, Rm, np.random.default_rng(193).standard_normal(Pm.shape[1])


def operator(slots, lines):
    A, x0, b, wants = problem(slots, lines)
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack()
    assert dA.stencil is not None and (dA.stencil.W, dA.stencil.umask) == (W, slots) and dA.stencil.hot >= 0
    assert ops._lib.lib().lmg_stencil_smooth_supported(slots)
    return dA


def packed_transfers():
    Pm, Rm, e = transfers()
    dP, dR = ops.DeviceCSR.from_scipy(Pm, DEV), ops.DeviceCSR.from_scipy(Rm, DEV)
    dP.pack(line_strides=(W, 193))
    dR.pack(line_strides=(W, 193))
    TP, TR = dP.prolong, dR.restrict
    assert TP is not None and (TP.W, TP.Wc, TP.nc) == (W, 193, 193 * 49)
    assert TR is not None and (TR.W, TR.Wc, TR.nc, TR.n) == (W, 193, 193 * 49, W * LINES)
    return dP, dR


@contextlib.contextmanager
def register_pass(dA, seg_lines=0, **keys):
    """The register pass with `seg_lines` lines per segment (0: chosen per launch) and the tune keys given."""
    with FC.register_pass(seg_lines), SV.tuned(**keys):
        assert ops._fused_kind(dA) is None
        yield


@pytest.mark.parametrize("slots", SLOTS, ids=IDS)
def test_fast_body_and_general_body_give_the_same_bits(slots):
    """Default keys: S = 1..3, with and without the residual, zero and non-zero iterate, first with the fast body where a
    wave qualifies, then with every wave on the general body.  Both equal the oracle, hence each other."""
    A, x0, b, wants = problem(slots, LINES)
    dA = operator(slots, LINES)
    for fast in (1, 0):
        with register_pass(dA, fused_fast=fast):
            FC.check_smoothing(("fused_fast", fast), dA, x0, b, wants)


@pytest.mark.parametrize("slots", SLOTS, ids=IDS)
def test_balance_of_the_slow_items(slots):
    """fused_balance off: uniform segments, no boundary items.  On: the boundary strips and the edge segments get
    fused_slow_pct per cent of a normal item's steps -- 10 drives that to its floor of 2 lines, 100 makes it a whole
    segment, i.e. no boundary items again."""
    A, x0, b, wants = problem(slots, LINES)
    dA = operator(slots, LINES)
    for balance, pct in ((0, 55), (1, 10), (1, 55), (1, 100)):
        with register_pass(dA, fused_balance=balance, fused_slow_pct=pct):
            FC.check_smoothing(("fused_balance", balance, "fused_slow_pct", pct), dA, x0, b, wants)


@pytest.mark.parametrize("slots", SLOTS, ids=IDS)
def test_segment_count_from_the_wanted_waves(slots):
    """With one wave wanted a segment is the whole strip; with 5120 and one halo as the floor it is 1 .. 4 lines."""
    A, x0, b, wants = problem(slots, LINES)
    dA = operator(slots, LINES)
    for waves in (1, 64, 5120):
        for halos in (1, 4):
            with register_pass(dA, fused_want_waves=waves, fused_floor_halos=halos):
                FC.check_smoothing(("fused_want_waves", waves, "fused_floor_halos", halos), dA, x0, b, wants)


@pytest.mark.parametrize("slots", SLOTS, ids=IDS)
def test_segment_count_of_the_three_sweep_transfer_passes(slots):
    """The passes of three sweeps with a transfer folded in take their wave count from fused_want_waves_rest3 (from a
    zero iterate: from fused_want_waves, set alike).  385 x 97 over 193 x 49."""
    A, x0, b, wants = problem(slots, LINES)
    dA = operator(slots, LINES)
    Pm, Rm, e = transfers()
    dP, dR = packed_transfers()
    for waves in (1, 64):
        for halos in (1, 4):
            with register_pass(dA, fused_want_waves_rest3=waves, fused_want_waves=waves, fused_floor_halos=halos):
                FC.check_pre(A, Rm, dA, dR, x0, b, sweeps=(3,))
                FC.check_post(A, Pm, dA, dP, x0, b, e, sweeps=(3,))


@pytest.mark.parametrize("slots", SLOTS, ids=IDS)
def test_edge_segments_around_their_threshold(slots):
    """The other strips get a first and a last segment of their own from  lines >= 2 * edge + seg_lines  on, with
    edge = max(HL + 10, slow).  With 7-line segments slow is 2 or 3 lines, so edge is 10 .. 14 lines for the halos
    HL = 0 .. 4 of these passes and the threshold is 27, 29, 31, 33 or 35 lines.  Every line count from 26 to 40: for every
    halo the decomposition without and with edge segments, and the first line count on either side."""
    for lines in range(26, 41):
        A, x0, b, wants = problem(slots, lines)
        dA = operator(slots, lines)
        with register_pass(dA, 7):
            FC.check_smoothing(("edge segments", lines), dA, x0, b, wants)


@pytest.mark.parametrize("slots", SLOTS, ids=IDS)
def test_segment_keys_of_the_transfer_passes(slots):
    """fused_seg_lines_prol / fused_seg_lines_rest override fused_seg_lines on the passes with a transfer folded in."""
    A, x0, b, wants = problem(slots, LINES)
    dA = operator(slots, LINES)
    Pm, Rm, e = transfers()
    dP, dR = packed_transfers()
    for seg in (3, 9):
        with register_pass(dA, 1000, fused_seg_lines_prol=seg, fused_seg_lines_rest=seg):
            FC.check_pre(A, Rm, dA, dR, x0, b)
            FC.check_post(A, Pm, dA, dP, x0, b, e)


@pytest.mark.parametrize("slots", SLOTS, ids=IDS)
def test_line_range_of_the_segment_key(slots):
    """fused_seg_lines applies to grids of fused_seg_min_lines .. fused_seg_max_lines lines: the 97-line grid inside the
    range (7-line segments), then above it and below it (segments chosen per launch).  Only the bits are asserted."""
    A, x0, b, wants = problem(slots, LINES)
    dA = operator(slots, LINES)
    for lo, hi in ((90, 100), (97, 97), (0, 96), (98, 1000)):
        with register_pass(dA, 7, fused_seg_min_lines=lo, fused_seg_max_lines=hi):
            FC.check_smoothing(("fused_seg_lines 7 for lines", lo, hi), dA, x0, b, wants)
