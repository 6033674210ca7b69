"""Every compiled packed-CSR sweep (csrc/pcsr.hip) against the CPU oracle on the CSR matrix, bit for bit (-m gpu).

The kernels: 3 modes x 2 column modes x 3 value modes x JU 1/3/5 on 512-row tiles, and JU 3/5 x VAL8/VAL64 on 128- and
64-row tiles.  The launcher picks ONE JU from the average row length; here pcsr_ju forces each, on matrices chosen so that
the builder's own rule (PackedCSR.from_csr) selects every value encoding and tile height, once with the columns it
chooses (uint16 on all of these) and once with int32 columns (the builder's colmode override):

  poisson_33        5-point Poisson 33 x 33, n = 1089: tiles of 512, 512 and 65 rows          VAL8,  512-row tiles
  int_values_1100   3 - 8 entries per row, integer values 1 .. 3000, every 7th row empty,
                    every 5th without a diagonal entry                                        VAL16, 512-row tiles
  tridiagonal       random values, n = 22100 (see below)                                      VAL64, 512-row tiles
  jittered_140      P.jittered_poisson_2d(140), n = 19881 (see below)                         VAL64, 128-row tiles
  cols20_300        20 random columns per row, random values                                  VAL64, 64-row tiles
  cols25_300        25 columns per row, values from a set of 50                               VAL8,  128-row tiles
  cols60_200        60 columns per row, values from a set of 50                               VAL8,  64-row tiles

The builder keeps raw fp64 values (VAL64) on tiles of 512 or 128 rows only for a matrix with more than 65536 distinct
values; with fewer it builds a 16-bit dictionary, or, where the rows are long, goes to raw values AND 64-row tiles.  A
tridiagonal matrix of 1100 rows or the jittered operator of a 31 x 31 grid has a few thousand values and gets VAL16 on
512-row tiles, so these two cases are the smallest of their kind with more than 65536 entries: 22100 rows (43 tiles and
one of 84 rows) and the 141 x 141 grid (a symmetric operator: every off-diagonal value occurs twice).  The small jittered
operator serves as the VAL16 twin forced onto 128-row tiles, which no kernel is built for.

Also: a 130 x 1100 SpMV (an inactive slot of a step gathers x at the tile's first column: x longer than the row count),
the two error statuses of lmg_pcsr_sweep with the fall-back of ops._sweep to plain CSR, and the guard in front of the two
timing probes pcsr_ju = 101 / 102, whose output is not the sweep's and which are therefore never run here."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sweep_variants as SV                                          # noqa: E402
from learnmultigrid_amd import _lib, ops, problems as P              # noqa: E402
from oracle import kernels as K                                      # noqa: E402  (checker only)

DEV = SV.DEV
ERR_ARG, ERR_CAPACITY = -1, -4
VAL8, VAL16, VAL64 = 0, 1, 2
JUS = (0, 1, 3, 5)
# name -> (value mode, tile height) the builder's rule must select
CASES = {
    "poisson_33": (VAL8, 512),
    "int_values_1100": (VAL16, 512),
    "tridiagonal": (VAL64, 512),
    "jittered_140": (VAL64, 128),
    "cols20_300": (VAL64, 64),
    "cols25_300": (VAL8, 128),
    "cols60_200": (VAL8, 64),
}


@functools.lru_cache(maxsize=None)
def matrix(name):
    rng = np.random.default_rng(len(name))
    if name == "poisson_33":
        return K.as_csr(P.poisson_2d_structured(32)[0])
    if name == "int_values_1100":
        n = 1100
        i = np.arange(n)
        lens = np.where(i % 7 == 3, 0, rng.integers(3, 9, n))
        A = SV.rows_matrix(n, n, lens, (lens > 0) & (i % 5 != 0), seed=3, values=np.arange(1, 3001))
        assert np.unique(A.data).size > 256
        return A
    if name == "tridiagonal":
        n = 22100
        A = K.as_csr(sp.diags([rng.standard_normal(n - 1), rng.standard_normal(n), rng.standard_normal(n - 1)], [-1, 0, 1]))
        assert np.unique(A.data).size > 65536 and A.nnz == 3 * n - 2
        return A
    if name in ("jittered_140", "jittered_30"):
        A = K.as_csr(P.jittered_poisson_2d(int(name.split("_")[1]), seed=7)[0])
        assert (np.unique(A.data).size > 65536) == (name == "jittered_140")
        return A
    if name in ("cols20_300", "cols25_300", "cols60_200", "cols255_256"):
        k, n = (int(v) for v in name[4:].split("_"))
        values = None if k in (20, 255) else np.random.default_rng(50).standard_normal(50)
        return SV.rows_matrix(n, n, np.full(n, k), np.ones(n, dtype=bool), seed=k, values=values)
    if name == "rect_130x1100":
        return SV.rows_matrix(130, 1100, np.full(130, 7), np.zeros(130, dtype=bool), seed=13)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def problem(name):
    return SV.Problem(matrix(name), seed=len(name) + 40)


def pcsr_operator(A, **overrides):
    """The operator with a packed twin built directly and nothing else, so that ops._sweep takes the PCSR branch."""
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    Pk = ops.PackedCSR.from_csr(dA, **overrides)
    assert Pk is not None
    dA.packed = Pk
    assert dA.patterns is None and dA.stencil is None and dA.sell is None and ops._PACKED_ENABLED
    return dA, Pk


def raw_sweep(mode, Pk, x, b, out, alpha=0.8, beta=0.0):
    """lmg_pcsr_sweep itself: its status."""
    tail = (ops._p(x), ops._p(b), ops._p(out), float(alpha), float(beta), None, None)
    return ops._twin_sweep(_lib.lib().lmg_pcsr_sweep, mode, Pk, tail)


@pytest.mark.parametrize("colmode", [None, 1], ids=["builder", "col32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_pcsr_kernel_bit_exact(name, colmode):
    ops.set_sell_enabled(False)
    try:
        pr = problem(name)
        dA, Pk = pcsr_operator(pr.A, colmode=colmode)
        valmode, tile_rows = CASES[name]
        assert (Pk.valmode, Pk.tile_rows) == (valmode, tile_rows), (name, Pk.valmode, Pk.tile_rows, Pk.ndict)
        assert Pk.colmode == (0 if colmode is None else 1)
        assert Pk.tile_cap == int(np.add.reduceat(np.diff(pr.A.indptr), np.arange(0, pr.A.shape[0], tile_rows)).max())
        for ju in JUS:                               # (on the short tiles the launcher runs 1 as 3)
            with SV.tuned(pcsr_ju=ju):
                SV.check_sweeps((name, colmode, "pcsr_ju", ju), dA, pr)
    finally:
        ops.set_sell_enabled(True)


@pytest.mark.parametrize("colmode", [None, 1], ids=["builder", "col32"])
def test_rectangular_spmv_gathers_beyond_the_row_count(colmode):
    pr = problem("rect_130x1100")
    dA, Pk = pcsr_operator(pr.A, colmode=colmode)
    assert (Pk.valmode, Pk.tile_rows, Pk.tile_cap) == (VAL16, 512, 910) and Pk.colmode == (0 if colmode is None else 1)
    for ju in (1, 3, 5):
        with SV.tuned(pcsr_ju=ju):
            SV.check_sweeps(("rect", colmode, ju), dA, pr, spmv_only=True)


def test_a_16_bit_dictionary_on_short_tiles_is_an_argument_error():
    """VAL16 exists on 512-row tiles only (the builder never asks for anything else): LMG_ERR_ARG, nothing written."""
    pr = problem("jittered_30")
    dA, Pk = pcsr_operator(pr.A, tile_rows=128)
    assert (Pk.valmode, Pk.tile_rows, Pk.colmode) == (VAL16, 128, 0)
    dx, db = SV.dev(pr.x), SV.dev(pr.b)
    for mode in (0, 1, 2):
        for ju in JUS:
            with SV.tuned(pcsr_ju=ju):
                out = SV.Guarded(pr.A.shape[0], pr.y0)
                assert raw_sweep(mode, Pk, dx, db, out.out) == ERR_ARG, (mode, ju)
                assert np.array_equal(out.result((mode, ju)), pr.y0)
    # the same operator as the builder packs it
    dA, Pk = pcsr_operator(pr.A)
    assert (Pk.valmode, Pk.tile_rows) == (VAL16, 512)
    SV.check_sweeps("jittered_30", dA, pr)


def test_a_tile_beyond_the_lds_is_a_capacity_error_and_falls_back_to_plain_csr():
    """255 entries per row, all distinct (256 rows: the smallest square that holds such rows): raw values on 64-row tiles
    of 16320 entries, about 160 KB of LDS.  lmg_pcsr_sweep answers LMG_ERR_CAPACITY and writes nothing; ops._sweep then
    runs the plain-CSR kernels, whose bits are the oracle's."""
    pr = problem("cols255_256")
    dA, Pk = pcsr_operator(pr.A)
    assert (Pk.valmode, Pk.tile_rows, Pk.colmode, Pk.tile_cap) == (VAL64, 64, 0, 64 * 255)
    dx, db = SV.dev(pr.x), SV.dev(pr.b)
    for mode in (0, 1, 2):
        out = SV.Guarded(pr.A.shape[0], pr.y0)
        assert raw_sweep(mode, Pk, dx, db, out.out) == ERR_CAPACITY, mode
        assert np.array_equal(out.result(mode), pr.y0)
    for ju in JUS:
        with SV.tuned(pcsr_ju=ju):
            SV.check_sweeps(("cols255_256", ju), dA, pr)


@pytest.mark.parametrize("name,overrides", [("int_values_1100", {}), ("cols25_300", {}), ("tridiagonal", {}),
                                            ("poisson_33", {"colmode": 1}), ("poisson_33", {"tile_rows": 128})],
                         ids=["val16", "val8_128", "val64", "val8_col32", "val8_col16_128"])
def test_the_timing_probes_are_refused_off_their_encoding(name, overrides):
    """pcsr_ju = 101 / 102 launch kernels that leave out the gathers of x (and the staging): timing probes whose output is
    not the sweep's (include/lmg.h).  They exist for uint16 columns, a uint8 dictionary and 512-row tiles; every other
    twin gets LMG_ERR_ARG and nothing is launched.  (On their own encoding they run, and are not run here.)"""
    pr = problem(name)
    dA, Pk = pcsr_operator(pr.A, **overrides)
    assert (Pk.colmode, Pk.valmode, Pk.tile_rows) != (0, VAL8, 512)
    dx, db = SV.dev(pr.x), SV.dev(pr.b)
    for probe in (101, 102):
        with SV.tuned(pcsr_ju=probe):
            for mode in (0, 1, 2):
                out = SV.Guarded(pr.A.shape[0], pr.y0)
                assert raw_sweep(mode, Pk, dx, db, out.out) == ERR_ARG, (probe, mode)
                assert np.array_equal(out.result((probe, mode)), pr.y0)
            with pytest.raises(ops.LmgError):
                ops.csr_jacobi(dA, dx, db, 0.8, SV.Guarded(pr.A.shape[0]).out)
