"""TEST-ONLY (-m gpu): the checkers of the fused grid passes that several GPU test modules share -- the Jacobi passes with a
transfer folded in against the oracle (check_pre, check_post), the Chebyshev passes against the two-launch path and the CPU
twin (check_plain, check_transfers, the histories of whole solves), the plain passes against precomputed oracle results
(jacobi_wants, check_smoothing) -- and the tune-key scopes they run under."""
import contextlib

import numpy as np
import scipy.sparse as sp
import torch

import chebyshev_ref as C
from learnmultigrid_amd import ops, problems as P
from learnmultigrid_amd.hierarchy import chebyshev_coefficients
from oracle import kernels as K
from support import DEV, dev, nan_vec


# ---- tune keys ---------------------------------------------------------------------------------------------------------------
def knobs_over(KNOBS):
    """The context manager `knobs(**kw)` of a test module: sets the tune keys given by keyword for the block and puts every
    key of KNOBS back to what it was afterwards."""
    class knobs:
        def __init__(self, **kw):
            self.kw = kw

        def __enter__(self):
            self.old = {k: ops.tune_get(k) for k in KNOBS}
            for k, v in self.kw.items():
                ops.tune_set(k, v)

        def __exit__(self, *exc):
            for k, v in self.old.items():
                ops.tune_set(k, v)

    return knobs


tile_knobs = knobs_over(("tile_hot_transfers", "tile_rows", "tile_rows_big", "tile_prol_wide_lines_hx"))
cheby_knobs = knobs_over(("tile_hot_transfers", "tile_rows", "tile_rows_big", "tile_prol_wide_lines_hx", "dia_rows"))
# every instantiation of the transfer passes: 16- / 32-line tiles, the correcting pass on 2 or 4 lines per wave
LAYOUTS = [dict(tile_rows=16, tile_rows_big=16), dict(tile_rows=32, tile_rows_big=32, tile_prol_wide_lines_hx=1 << 30),
           dict(tile_rows=32, tile_rows_big=32, tile_prol_wide_lines_hx=0)]


@contextlib.contextmanager
def register_pass(seg_lines):
    """stencil_smooth on the register pass (levels of this size run the tiled one), `seg_lines` lines per segment."""
    try:
        ops.set_tiled_enabled(False)
        ops.tune_set("fused_seg_lines", seg_lines)
        yield
    finally:
        ops.tune_set("fused_seg_lines", 0)
        ops.set_tiled_enabled(True)


# ---- operators ---------------------------------------------------------------------------------------------------------------
def nested_pair(Wf, Hf):
    """P between the Wf x Hf grid and the ((Wf + 1) / 2) x ((Hf + 1) / 2) grid -- the tensor product of the 1-D
    interpolations along y and x -- and its transpose."""
    Pm = sp.kron(P.geometric_interpolator_1d(Hf), P.geometric_interpolator_1d(Wf), format="csr")
    Pm.sort_indices()
    return K.as_csr(Pm), K.as_csr(sp.csr_matrix(Pm.T))


# ---- the Jacobi passes ---------------------------------------------------------------------------------------------------------
def first_diff(got, want):
    return np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:8]


def jacobi_wants(A, x0, b):
    """(omega, zero iterate, sweeps) -> (J^S x, b - A J^S x) of the oracle: computed once per operator."""
    n = A.shape[0]
    out = {}
    for omega in (0.8, 1.0):
        for zero in (False, True):
            w = np.zeros(n) if zero else x0.copy()
            for S in (1, 2, 3):
                w = K.jacobi(A, w, b, omega)
                out[omega, zero, S] = (w, K.residual(A, w, b)[0])
    return out


def check_smoothing(tag, dA, x0, b, wants):
    """stencil_smooth for the sweeps 1..3, with and without the residual, zero and non-zero iterate, omega 0.8 and 1.0."""
    n = dA.shape[0]
    dx, db = dev(x0), dev(b)
    for (omega, zero, S), (want, wr) in wants.items():
        for resid in (False, True):
            out, r = nan_vec(n), (nan_vec(n) if resid else None)
            ops.stencil_smooth(dA, None if zero else dx, db, omega, S, out, r)
            got = out.cpu().numpy()
            assert not np.isnan(got).any(), (tag, omega, S, zero, resid, np.flatnonzero(np.isnan(got))[:8])
            assert np.array_equal(got, want), (tag, omega, S, zero, resid, first_diff(got, want))
            if resid:
                gr = r.cpu().numpy()
                assert np.array_equal(gr, wr), (tag, omega, S, zero, "residual", first_diff(gr, wr))


def check_pre(A, Rm, dA, dR, x0, b, sweeps=(1, 2, 3), zeros=(False, True)):
    n, nc = A.shape[0], Rm.shape[0]
    for zero in zeros:
        want = np.zeros(n) if zero else x0.copy()
        for S in range(1, max(sweeps) + 1):
            want = K.jacobi(A, want, b, 0.8)
            if S not in sweeps:
                continue
            wbc = K.spmv(Rm, K.residual(A, want, b)[0])
            out = torch.full((n,), np.nan, dtype=torch.float64, device=DEV)
            bc = torch.full((nc,), np.nan, dtype=torch.float64, device=DEV)
            ops.stencil_smooth(dA, None if zero else dev(x0), dev(b), 0.8, S, out, None, restrict=(dR, bc))
            assert np.array_equal(out.cpu().numpy(), want), (n, S, zero)
            got = bc.cpu().numpy()
            assert np.array_equal(got, wbc), (n, S, zero, np.flatnonzero(got != wbc)[:8])


def check_post(A, Pm, dA, dP, x0, b, e, sweeps=(1, 2, 3)):
    n = A.shape[0]
    want = K.spmv(Pm, e, x0.copy(), 1.0, 1.0)
    for S in range(1, max(sweeps) + 1):
        want = K.jacobi(A, want, b, 0.8)
        if S not in sweeps:
            continue
        out = torch.full((n,), np.nan, dtype=torch.float64, device=DEV)
        ops.stencil_smooth(dA, dev(x0), dev(b), 0.8, S, out, None, prolong=(dP, dev(e)))
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (n, S, np.flatnonzero(got != want)[:8])


# ---- the Chebyshev passes ------------------------------------------------------------------------------------------------------
def two_launch(dA, x0, b, coef):
    """The step as every format without a fused pass runs it: residual launch + lmg_cheby_update per sweep."""
    n = dA.shape[0]
    x = torch.zeros(n, dtype=torch.float64, device=DEV) if x0 is None else dev(x0)
    dinv = ops.csr_inverse_diagonal(dA)
    d, r, db = nan_vec(n), nan_vec(n), dev(b)
    for k, (a, c) in enumerate(coef):
        ops.csr_residual_norm2(dA, x, db, r, None, None)
        ops.cheby_update(a, c, dinv, r, d, x, first=(k == 0))
    return x.cpu().numpy()


def check_plain(A, dA, x0, b, lmax, ratio=4.0):
    """plain, + residual, zero iterate: tiled pass == two-launch path == twin for the degrees 1..3."""
    n = A.shape[0]
    for S in (1, 2, 3):
        coef = chebyshev_coefficients(lmax, ratio, S)
        for zero in (False, True):
            want = C.cheby_step(A, np.zeros(n) if zero else x0, b, coef)
            wr, _ = K.residual(A, want, b)
            unfused = two_launch(dA, None if zero else x0, b, coef)
            assert np.array_equal(unfused, want), (n, S, zero, "two-launch path vs twin")
            for resid in (False, True):
                out, r = nan_vec(n), (nan_vec(n) if resid else None)
                ops.stencil_cheby(dA, None if zero else dev(x0), dev(b), coef, out, r)
                got = out.cpu().numpy()
                assert not np.isnan(got).any(), (n, S, zero, resid)
                assert np.array_equal(got, want), (n, S, zero, resid, np.flatnonzero(got != want)[:8])
                assert np.array_equal(got, unfused)
                if resid:
                    assert np.array_equal(r.cpu().numpy(), wr), (n, S, zero)
        if S == 1:          # degree 1 is weighted Jacobi with omega = 1 / theta: the oracle's sweep and the Jacobi pass
            omega = coef[0][1]
            assert np.array_equal(C.cheby_step(A, x0, b, coef), K.jacobi(A, x0, b, omega))
            out = nan_vec(n)
            ops.stencil_smooth(dA, dev(x0), dev(b), omega, 1, out)
            assert np.array_equal(out.cpu().numpy(), C.cheby_step(A, x0, b, coef))


def check_transfers(A, Pm, Rm, dA, dP, dR, x0, b, e, lmax):
    n, nc = A.shape[0], Rm.shape[0]
    for S in (1, 2, 3):
        coef = chebyshev_coefficients(lmax, 4.0, S)
        for zero in (False, True):                                   # REST (and ZERO + REST)
            want = C.cheby_step(A, np.zeros(n) if zero else x0, b, coef)
            wbc = K.spmv(Rm, K.residual(A, want, b)[0])
            out, bc = nan_vec(n), nan_vec(nc)
            ops.stencil_cheby(dA, None if zero else dev(x0), dev(b), coef, out, None, restrict=(dR, bc))
            assert np.array_equal(out.cpu().numpy(), want), (n, S, zero, "restrict")
            got = bc.cpu().numpy()
            assert np.array_equal(got, wbc), (n, S, zero, np.flatnonzero(got != wbc)[:8])
        xe = K.spmv(Pm, e, x0.copy(), 1.0, 1.0)                      # PROL
        want = C.cheby_step(A, xe, b, coef)
        out = nan_vec(n)
        ops.stencil_cheby(dA, dev(x0), dev(b), coef, out, None, prolong=(dP, dev(e)))
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (n, S, "prolong", np.flatnonzero(got != want)[:8])
        assert np.array_equal(got, two_launch(dA, xe, b, coef))


def cheby_histories(H, rhs, cycles, degree, shape="V", graph=False):
    fine = H.levels[0]
    with torch.cuda.stream(H.stream):
        fine.b.copy_(dev(rhs.ravel()))
        ops.zero(fine.x)
        g = H.captured_cycle("Chebyshev", degree, 1.0, "lexicographic", shape=shape) if graph else None
        norms = []
        for _ in range(cycles):
            norms.append(H.residual_norm())
            if g is not None:
                g.launch()
            else:
                H.cycle("Chebyshev", degree, shape=shape)
        norms.append(H.residual_norm())
        x = fine.x.cpu().numpy().copy()
    return np.array(norms), x


def cheby_twin_history(A, rhs, hier, cycles, degree, shape="V", H=None):
    """The twin's history.  H: solve the coarsest level with that hierarchy's own direct solver (Hierarchy.coarse_solve) --
    the twin restates the smoother and the cycle, not the direct solver, and two direct solvers differ by rounding noise
    that a pointwise relative comparison would meet a few cycles before convergence."""
    ref = C.ChebyCycle.galerkin(A, hier)
    if H is not None:
        last = H.levels[-1]

        def coarse(rc):
            with torch.cuda.stream(H.stream):
                last.b.copy_(dev(rc))
                H.coarse_solve()
                return last.x.cpu().numpy().copy()

        ref.coarse = coarse
    b = np.asarray(rhs, dtype=float).ravel()
    x = np.zeros(A.shape[0])
    out = [np.sqrt(K.residual(K.as_csr(A), x, b)[1])]
    for _ in range(cycles):
        x = ref.cycle(x, b, degree=degree, shape=shape)
        out.append(np.sqrt(K.residual(K.as_csr(A), x, b)[1]))
    return np.array(out), x, ref
