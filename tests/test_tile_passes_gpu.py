"""The LDS-tiled smoothing passes with a grid transfer folded in (csrc/stencil_tile.hip), bitwise against the oracle:
the pre-smoothing pass with the restriction (b_c = R (b - A J^S x)) and the post-smoothing pass with the correction
(J^S (x + P e)).  Level 1 of cfg#4 itself (the 2049^2 9-point Galerkin operator), then every instantiation -- hot
transfers on and off (tile_hot_transfers), 16- and 32-line tiles, two and four lines per wave -- forced onto small
and odd grids, grids less than two tiles wide, and the pattern-table paths of P and R."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fused_checks import LAYOUTS, check_post, check_pre, tile_knobs as knobs   # noqa: E402
from learnmultigrid_amd import ops                  # noqa: E402
from support import DEV, dev, operators             # noqa: E402


def packed(A, Pm, Rm):
    dA, dP, dR = (ops.DeviceCSR.from_scipy(M, DEV) for M in (A, Pm, Rm))
    for d in (dA, dP, dR):
        d.pack()
    assert ops._fused_kind(dA) == "tile"
    assert ops.stencil_smooth_prolong_available(dA, dP) and ops.stencil_smooth_restrict_available(dA, dR)
    return dA, dP, dR


@pytest.fixture(scope="module")
def level1():
    """Level 1 of cfg#4: the 2049^2 9-point Galerkin operator and the transfers to 1025^2."""
    A, Pm, Rm = operators(2049, "9pt")
    dA, dP, dR = packed(A, Pm, Rm)
    rng = np.random.default_rng(2049)
    n, nc = A.shape[0], Pm.shape[1]
    return A, Pm, Rm, dA, dP, dR, rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(nc)


def test_level1_pre_smoothing_with_the_restriction(level1):
    A, Pm, Rm, dA, dP, dR, x0, b, e = level1
    assert dR.restrict.hot >= 0
    check_pre(A, Rm, dA, dR, x0, b)


def test_level1_post_smoothing_with_the_correction(level1):
    A, Pm, Rm, dA, dP, dR, x0, b, e = level1
    assert min(dP.prolong._hot_pairs) >= 0
    check_post(A, Pm, dA, dP, x0, b, e)


def test_level1_hot_transfers_match_the_previous_kernels(level1):
    """The same bits with tile_hot_transfers off (the kernels that carry the transfers on every fine element)."""
    A, Pm, Rm, dA, dP, dR, x0, b, e = level1
    n, nc = A.shape[0], Pm.shape[1]
    outs = {}
    for hx in (0, 1):
        with knobs(tile_hot_transfers=hx):
            y, z = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, dtype=torch.float64, device=DEV)
            bc = torch.empty(nc, dtype=torch.float64, device=DEV)
            ops.stencil_smooth(dA, None, dev(b), 0.8, 3, y, None, restrict=(dR, bc))
            ops.stencil_smooth(dA, y, dev(b), 0.8, 3, z, None, prolong=(dP, dev(e)))
            outs[hx] = [t.cpu().numpy() for t in (y, bc, z)]
    for a, c in zip(outs[0], outs[1]):
        assert np.array_equal(a, c)


# grids: odd and uneven sizes, widths that are no multiple of a tile's inner part, 65 / 99 columns (less than two
# 64-column tiles: the correction finds its coarse window by division)
CASES = [(65, "5pt"), (99, "5pt"), (99, "9pt"), (769, "5pt"), (769, "9pt"), (1029, "9pt"), (1537, "5pt")]


@pytest.mark.parametrize("side,kind", CASES)
@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
def test_transfer_passes_on_small_grids(side, kind, layout):
    A, Pm, Rm = operators(side, kind)
    dA, dP, dR = packed(A, Pm, Rm)
    rng = np.random.default_rng(side + layout)
    n, nc = A.shape[0], Pm.shape[1]
    x0, b, e = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(nc)
    with knobs(tile_hot_transfers=1, **LAYOUTS[layout]):
        check_pre(A, Rm, dA, dR, x0, b)
        check_post(A, Pm, dA, dP, x0, b, e)


@pytest.mark.parametrize("side,kind", [(99, "9pt"), (769, "9pt"), (1029, "5pt")])
def test_transfer_passes_through_the_pattern_tables(side, kind):
    """No frequent pattern of R / pair of P: every coarse row and every correction through the pattern table."""
    A, Pm, Rm = operators(side, kind)
    dA, dP, dR = packed(A, Pm, Rm)
    rng = np.random.default_rng(side)
    n, nc = A.shape[0], Pm.shape[1]
    x0, b, e = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(nc)
    TR, TP = dR.restrict, dP.prolong
    hot, pairs = TR.hot, (TP._hot_pairs[0], TP._hot_pairs[1])
    try:
        TR.hot = -1
        TP._hot_pairs[0] = TP._hot_pairs[1] = -1
        for layout in LAYOUTS:
            with knobs(tile_hot_transfers=1, **layout):
                check_pre(A, Rm, dA, dR, x0, b, sweeps=(1, 3))
                check_post(A, Pm, dA, dP, x0, b, e, sweeps=(2,))
    finally:
        TR.hot = hot
        TP._hot_pairs[0], TP._hot_pairs[1] = pairs
