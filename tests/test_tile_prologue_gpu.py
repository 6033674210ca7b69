"""The prologue of the LDS-tiled passes (csrc/stencil_tile.hip: every global load requested before any is used) at the
smallest shapes where it can go wrong, bitwise against oracle.kernels (jacobi, residual, spmv):

  * pattern tables longer than one 512-thread block: 9-point operators whose rows are scaled in groups until the stencil
    twin holds 57 .. 64 patterns (more than 512 / 9), and restrictions scaled the same way, on 16-line tiles -- the thread
    that stages element t of a table also has to stage element t + 512;
  * rows without a usable diagonal (they copy x) and live boundary rows with missing slots next to bands of the frequent
    pattern, so that waves of one workgroup take the scalar-register path and the table path side by side;
  * a grid narrower than two tiles (33 x 33, coarse 17 x 17: the correction finds its window by division), one of three
    tiles by three and more (129 x 129) and a rectangle (131 x 45): first and last tiles load from clamped addresses and
    hold elements outside the lines that are rows all the same;
  * every form: plain S = 1 .. 3 with and without the residual from a zero and a non-zero iterate, the correcting, the
    restricting and the turnaround pass, a Chebyshev step of degree 2 -- with tile_hot_transfers 0 and 1 on 16- and
    32-line tiles, and the correcting pass on four lines per wave.

Outputs start as NaN: an element that is never stored shows."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import chebyshev_ref as C                                            # noqa: E402  (checker only)
import grid_ops as G                                                 # noqa: E402
from learnmultigrid_amd import ops, problems as P                    # noqa: E402
from oracle import kernels as K                                      # noqa: E402  (checker only)
from fused_checks import knobs_over                                  # noqa: E402
from support import DEV, dev, nan_vec                                # noqa: E402

KNOBS = ("tile_hot_transfers", "tile_rows", "tile_rows_big", "tile_prol_wide_lines", "tile_prol_wide_lines_hx")
knobs = knobs_over(KNOBS)
OMEGA = 0.8
GRIDS = {"narrow": (33, 33), "wide": (129, 129), "rect": (131, 45)}


def first_diff(got, want):
    return np.flatnonzero(~(got == want))[:8]


@pytest.fixture(scope="module", autouse=True)
def tiled_from_the_first_row():
    """33 x 33 is below the size from which the hierarchy picks the tiled pass; the kernels take any size."""
    old = ops.TILED_MIN_ROWS
    ops.TILED_MIN_ROWS = 0
    yield
    ops.TILED_MIN_ROWS = old


def scaled_in_groups(M, Wg, Hg, groups):
    """diag(s) M with s = 1 on the rim of the Wg x Hg grid of M's rows and on bands of three lines out of six, and one
    of `groups` - 1 other values on the interior rows between them: every group of interior rows is a pattern of its
    own, the bands keep the frequent one on whole wave lines."""
    idx = np.arange(Wg * Hg)
    y, x = idx // Wg, idx % Wg
    inner = (x > 0) & (x < Wg - 1) & (y > 0) & (y < Hg - 1)
    between = inner & ((y // 3) % 2 == 1)
    g = np.where(between, 1 + (np.cumsum(between) - 1) % (groups - 1), 0)      # (in turn: every group has its rows)
    assert np.unique(g).size == groups
    s = 1.0 + g / 64.0
    return K.as_csr(sp.csr_matrix(sp.diags(s) @ M)), g


def nested_pair(Wf, Hf):
    """P between the Wf x Hf grid and the ((Wf + 1) / 2) x ((Hf + 1) / 2) grid and its transpose."""
    Pm = sp.kron(P.geometric_interpolator_1d(Hf), P.geometric_interpolator_1d(Wf), format="csr")
    Pm.sort_indices()
    return K.as_csr(Pm), K.as_csr(sp.csr_matrix(Pm.T))


class Case:
    """One grid: the operator and the transfers on the device, and every expected vector, computed once."""

    def __init__(self, name):
        Wf, Hf = GRIDS[name]
        Wc, Hc = (Wf + 1) // 2, (Hf + 1) // 2
        A0 = G.grid_op(Wf, Hf, 0x1FF, "const", seed=Wf)              # live boundary rows: 8 patterns with missing slots
        A, g = scaled_in_groups(A0, Wf, Hf, 52)
        # rows without a diagonal entry, inside the bands of the frequent pattern and on the rim
        self.nodiag = np.flatnonzero((g == 0) & (np.arange(Wf * Hf) % 37 == 5))[:40] if name == "wide" else np.array([], int)
        if self.nodiag.size:
            A = A.tolil()
            for i in self.nodiag:
                A[i, i] = 0.0
            A = sp.csr_matrix(A)
            A.eliminate_zeros()
            A = K.as_csr(A)
        Pm, R0 = nested_pair(Wf, Hf)
        Rm, _ = scaled_in_groups(R0, Wc, Hc, 52)
        self.A, self.Pm, self.Rm = A, Pm, Rm
        self.n, self.nc = A.shape[0], Pm.shape[1]
        assert (self.n, self.nc) == (Wf * Hf, Wc * Hc)
        self.dA, self.dP, self.dR = (ops.DeviceCSR.from_scipy(M, DEV) for M in (A, Pm, Rm))
        self.dA.pack()
        self.dP.pack(line_strides=(Wf, Wc))
        self.dR.pack(line_strides=(Wf, Wc))
        rng = np.random.default_rng(Wf * Hf)
        self.x0, self.b, self.e = rng.standard_normal(self.n), rng.standard_normal(self.n), rng.standard_normal(self.nc)
        A, x0, b, e = self.A, self.x0, self.b, self.e
        # plain: J^S from x0 and from zero, with the residual
        self.plain = {}
        for zero in (False, True):
            want = np.zeros(self.n) if zero else x0.copy()
            for S in (1, 2, 3):
                want = K.jacobi(A, want, b, OMEGA)
                self.plain[zero, S] = (want, K.residual(A, want, b)[0])
        self.pre = {k: K.spmv(Rm, r) for k, (_, r) in self.plain.items()}           # R (b - A J^S x)
        self.post = {}                                                                 # J^S (x0 + P e)
        want = K.spmv(Pm, e, x0.copy(), 1.0, 1.0)
        for S in (1, 2, 3):
            want = K.jacobi(A, want, b, OMEGA)
            self.post[S] = want
        self.turn = (self.post[3], K.spmv(Rm, K.residual(A, self.post[3], b)[0]))     # 1 + 2 sweeps, then R
        self.coef = C.coefficients(C.gershgorin(A), 4.0, 2)
        ch = C.cheby_step(A, x0, b, self.coef)
        self.cheby = (ch, K.residual(A, ch, b)[0])
        self.cheby_pre = K.spmv(Rm, self.cheby[1])
        self.cheby_post = C.cheby_step(A, K.spmv(Pm, e, x0.copy(), 1.0, 1.0), b, self.coef)


_cases = {}


@pytest.fixture(params=sorted(GRIDS))
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


def test_the_cases_are_what_they_claim(case):
    """More patterns than one block stages in one go, in A and in R; the tiled pass; rows that copy x where asked for."""
    S, TP, TR = case.dA.stencil, case.dP.prolong, case.dR.restrict
    assert S is not None and S.umask == 0x1FF and 57 <= S.npat <= 64 and S.npat * 9 > 512
    assert TR is not None and 57 <= TR.npat <= 64 and TR.npat * 9 > 512
    assert TP is not None and S.hot >= 0 and TR.hot >= 0 and min(TP._hot_pairs) >= 0
    assert ops._fused_kind(case.dA) == "tile"
    assert ops.stencil_smooth_prolong_available(case.dA, case.dP) and ops.stencil_smooth_restrict_available(case.dA, case.dR)
    assert ops.stencil_smooth_turnaround_available(case.dA, case.dP, case.dR)
    mask = S.st_mask.cpu().numpy()
    assert (mask != 0x1FF).sum() >= 8                                # the rim: patterns with missing slots
    if case.nodiag.size:
        assert (case.A.diagonal()[case.nodiag] == 0.0).all() and ((mask & 16) == 0).any()
        assert np.array_equal(case.plain[False, 3][0][case.nodiag], case.x0[case.nodiag])     # such rows copy x


@pytest.mark.parametrize("rows", [16, 32])
def test_plain_passes(case, rows):
    c = case
    with knobs(tile_rows=rows, tile_rows_big=rows):
        for (zero, S), (want, wr) in c.plain.items():
            for resid in (False, True):
                out, r = nan_vec(c.n), (nan_vec(c.n) if resid else None)
                ops.stencil_smooth(c.dA, None if zero else dev(c.x0), dev(c.b), OMEGA, S, out, r)
                got = out.cpu().numpy()
                assert np.array_equal(got, want), (S, zero, resid, first_diff(got, want))
                if resid:
                    got = r.cpu().numpy()
                    assert np.array_equal(got, wr), (S, zero, first_diff(got, wr))


@pytest.mark.parametrize("rows", [16, 32])
@pytest.mark.parametrize("hx", [0, 1])
def test_restricting_pass(case, hx, rows):
    c = case
    with knobs(tile_hot_transfers=hx, tile_rows=rows, tile_rows_big=rows):
        for (zero, S), (want, _) in c.plain.items():
            out, bc = nan_vec(c.n), nan_vec(c.nc)
            ops.stencil_smooth(c.dA, None if zero else dev(c.x0), dev(c.b), OMEGA, S, out, None, restrict=(c.dR, bc))
            got = out.cpu().numpy()
            assert np.array_equal(got, want), (S, zero, first_diff(got, want))
            got = bc.cpu().numpy()
            assert np.array_equal(got, c.pre[zero, S]), (S, zero, first_diff(got, c.pre[zero, S]))


# 16- and 32-line tiles on two lines per wave, 32-line tiles on four
POST_LAYOUTS = [dict(tile_rows=16, tile_rows_big=16), dict(tile_rows=32, tile_rows_big=32),
                dict(tile_rows=32, tile_rows_big=32, tile_prol_wide_lines=0, tile_prol_wide_lines_hx=0)]


@pytest.mark.parametrize("layout", range(len(POST_LAYOUTS)))
@pytest.mark.parametrize("hx", [0, 1])
def test_correcting_pass(case, hx, layout):
    c = case
    with knobs(tile_hot_transfers=hx, **POST_LAYOUTS[layout]):
        for S, want in c.post.items():
            out = nan_vec(c.n)
            ops.stencil_smooth(c.dA, dev(c.x0), dev(c.b), OMEGA, S, out, None, prolong=(c.dP, dev(c.e)))
            got = out.cpu().numpy()
            assert np.array_equal(got, want), (S, first_diff(got, want))


@pytest.mark.parametrize("rows", [16, 32])
@pytest.mark.parametrize("hx", [0, 1])
def test_turnaround_pass(case, hx, rows):
    c = case
    with knobs(tile_hot_transfers=hx, tile_rows=rows, tile_rows_big=rows):
        out, bc = nan_vec(c.n), nan_vec(c.nc)
        ops.stencil_smooth_turnaround(c.dA, dev(c.x0), dev(c.b), OMEGA, 1, 2, out, (c.dP, dev(c.e)), (c.dR, bc))
        got = out.cpu().numpy()
        assert np.array_equal(got, c.turn[0]), first_diff(got, c.turn[0])
        got = bc.cpu().numpy()
        assert np.array_equal(got, c.turn[1]), first_diff(got, c.turn[1])


@pytest.mark.parametrize("rows", [16, 32])
@pytest.mark.parametrize("hx", [0, 1])
def test_chebyshev_degree_two(case, hx, rows):
    c = case
    assert ops.stencil_cheby_available(c.dA)
    with knobs(tile_hot_transfers=hx, tile_rows=rows, tile_rows_big=rows):
        out, r = nan_vec(c.n), nan_vec(c.n)
        ops.stencil_cheby(c.dA, dev(c.x0), dev(c.b), c.coef, out, r)
        assert np.array_equal(out.cpu().numpy(), c.cheby[0]) and np.array_equal(r.cpu().numpy(), c.cheby[1])
        out, bc = nan_vec(c.n), nan_vec(c.nc)
        ops.stencil_cheby(c.dA, dev(c.x0), dev(c.b), c.coef, out, None, restrict=(c.dR, bc))
        got = bc.cpu().numpy()
        assert np.array_equal(out.cpu().numpy(), c.cheby[0]) and np.array_equal(got, c.cheby_pre), first_diff(got, c.cheby_pre)
        out = nan_vec(c.n)
        ops.stencil_cheby(c.dA, dev(c.x0), dev(c.b), c.coef, out, None, prolong=(c.dP, dev(c.e)))
        got = out.cpu().numpy()
        assert np.array_equal(got, c.cheby_post), first_diff(got, c.cheby_post)
