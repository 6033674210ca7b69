"""Torch-facing wrappers of the C ABI (include/lmg.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every
arithmetic step is a hand-written gfx950 kernel reached through ctypes.  The same
Python callables back the `torch.ops.lmg.*` ops (torch_ops.py; register_torch_ops() here
registers them) and the solver's internal calls.

What lives here: DeviceCSR and its pack() policy -- which of the storage twins of twins.py an operator gets --, every
enable switch and size threshold that picks a kernel, and one wrapper per entry point: sweeps, fused smoothing passes,
sweeps on blocks of right-hand sides, Gauss-Seidel, vectors, dense blocks, SpGEMM, hipGraph capture.  The twins themselves -- their formats, their construction
and the C arguments that describe them -- are in twins.py and re-exported here under their old names.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import LmgError, check
from .twins import (F32, F64, I32, ColorSell, DiaTwin, PackedCSR, ProlongTwin, RestrictTwin, RowPatterns, SellCSR,  # noqa: F401
                    StencilTwin, _p, _s, census_stride, check_values)


def _vec_ok(*ts):
    for t in ts:
        if t is None:
            continue
        if t.dtype != F64 or not t.is_contiguous() or not t.is_cuda:
            raise TypeError("expected contiguous float64 device tensors, got %s %s contiguous=%s"
                            % (t.dtype, t.device, t.is_contiguous()))


class DeviceCSR:
    """CSR matrix resident in HBM: int32 rowptr[n+1], int32 colidx[nnz], fp64 vals[nnz]."""

    __slots__ = ("rowptr", "colidx", "vals", "shape", "nnz", "packed", "patterns", "sell", "stencil", "prolong", "restrict",
                 "dia", "values", "twin_values")

    def __init__(self, rowptr, colidx, vals, shape):
        if rowptr.dtype != I32 or colidx.dtype != I32 or vals.dtype != F64:
            raise TypeError("DeviceCSR wants int32 indices and float64 values")
        if rowptr.numel() != shape[0] + 1 or colidx.numel() != vals.numel():
            raise ValueError("inconsistent CSR arrays")
        self.rowptr, self.colidx, self.vals = rowptr.contiguous(), colidx.contiguous(), vals.contiguous()
        self.shape = (int(shape[0]), int(shape[1]))
        self.nnz = int(vals.numel())
        self.packed = None           # PackedCSR twin used by the sweeps once pack() was called
        self.patterns = None         # RowPatterns twin (matrices with repeating rows), preferred
        self.sell = None             # SellCSR twin (long rows with all-distinct values)
        self.stencil = None          # StencilTwin view of `patterns` (3x3 grid stencils), preferred
        self.prolong = None          # ProlongTwin view of `patterns` (2x2-window grid prolongations)
        self.restrict = None         # RestrictTwin view of `patterns` (their transposes)
        self.dia = None              # DiaTwin (grid operators with per-row values): fused smoothing passes only
        self.values = "f64"          # what pack() was last asked for: "f64" | "f32" (repack_values honours it)
        self.twin_values = "f64"     # what the twins hold: "f32" = A32 = double(float(A)), value by value

    def pack(self, patterns=None, line_strides=None, values=None):
        """Build (once) the lossless twin the sweep kernels prefer; keeps the CSR arrays.
        Row patterns (RowPatterns) when the rows repeat -- assembled grid operators --, else the
        packed CSR (PackedCSR).  patterns=False forces the packed CSR, None = module default.
        line_strides: see RowPatterns.grid_map_candidates (transfers between non-square blocks of grid lines).
        values: "f64" | "f32", None = what the matrix remembers from an earlier pack() ("f64" at first).  "f32" (a cycle
        used as a preconditioner): every twin of the matrix represents A32 = double(float(A)), value by value -- the SELL
        and DIA twins store fp32 values, which the kernels widen when they load them; the row-pattern and packed twins
        keep their formats and widths (one byte per row, dictionary-coded or raw fp64 values) and are built from the
        rounded values, so that every launch on the matrix applies the same operator.  The CSR arrays keep the fp64 values
        (the Galerkin products and the coarse factorisation read them).  A matrix with a value that fails the range rule
        (SellCSR) gets fp64 twins as a whole: twin_values says what the twins hold."""
        if values is not None:
            check_values(values)
        if not self.vals.is_cuda:
            return None
        src = self
        if values is not None and values != self.values:
            self.values = values
            src = self._retarget()
        elif self.twin_values == "f32":
            src = self.cycle_source()
        # src: what the formats that do not narrow are built from
        vkw = {} if self.twin_values == "f64" else {"values": "f32"}
        if patterns is None:
            patterns = _PATTERNS_ENABLED
        if patterns and self.patterns is None and self.packed is None and self.sell is None:
            if self.shape[0] == self.shape[1]:
                self.patterns = RowPatterns.from_csr(src)
            else:
                # rectangular grid operators (transfers): row patterns relative to a column-base map
                for gm in (RowPatterns.grid_map_candidates(self.shape, line_strides) if _GRID_MAPS_ENABLED else []):
                    self.patterns = RowPatterns.from_csr(src, gm)
                    if self.patterns is not None:
                        break
            self._derive_grid_twins()
        if patterns and self.patterns is not None:
            return self.patterns
        if self.sell is not None:
            return self.sell
        if self.packed is None:
            if self.dia is None and _DIA_ENABLED and self.shape[0] == self.shape[1]:
                # variable-coefficient grid operators: slot arrays for the fused smoothing passes, next to the
                # packed CSR that serves the single sweeps / SpMV
                self.dia = DiaTwin.from_csr(self, **vkw)
            self.packed = PackedCSR.from_csr(src)
            # long rows whose values do not fit a dictionary: the sliced-ELL twin reads them without
            # LDS staging (the packed kernel's row-strided LDS walk is bank-conflict-bound there)
            pk = self.packed
            long_raw = pk is not None and pk.valmode == 2 and pk.tile_rows < 512
            unpackable = pk is None and self.nnz > 0           # rows longer than 255 entries (dense-ish operators)
            if _SELL_ENABLED and (long_raw or unpackable) and self.nnz >= SELL_MIN_AVG * self.shape[0]:
                self.sell = SellCSR.from_csr(self, **vkw)
                if self.sell is not None:
                    self.packed = None
                    return self.sell
        return self.packed

    def _derive_grid_twins(self):
        """stencil, prolong, restrict: the window views of `patterns` the fused passes read (None where it has none)."""
        self.stencil, self.prolong, self.restrict = (
            T.from_patterns(self.patterns, self.shape) if _STENCIL_ENABLED else None
            for T in (StencilTwin, ProlongTwin, RestrictTwin))
        S = self.stencil
        if S is not None and S.n >= min(FUSED_TRANSFER_MIN_ROWS, REG_PROLONG_MIN_ROWS, REG_RESTRICT_MIN_ROWS):
            # a level that may fold its transfers into the register pass: whether it has entries across a line end (two
            # device -> host reads) is asked in every cycle -- decided now, never while a hipGraph is being captured
            S.line_end_coupling

    def invalidate_packed(self):
        self.packed = self.patterns = self.sell = self.stencil = self.prolong = self.restrict = self.dia = None

    def _rounded(self):
        """The values rounded to fp32 and widened again (a new tensor), or None when one of them fails the range rule of
        the fp32 twins: other than 0 and not finite, or rounded to +-inf, a subnormal or zero.  (Library elementwise kernels:
        only a matrix packed with values="f32" ever comes here, at setup.)"""
        v = self.vals
        r = v.to(F32).to(F64)
        m = r.abs()
        bad = (v != 0) & ~((m >= float(np.finfo(np.float32).tiny)) & (m <= float(np.finfo(np.float32).max)))
        return None if bool(bad.any()) else r

    def _retarget(self):
        """Decide what the twins hold from what pack() was asked for and the values as they are now -- "f32" where every
        value passes the range rule --, drop twins of the other kind, and return the matrix the formats that do not narrow
        are built from (cycle_source, made once)."""
        r = self._rounded() if self.values == "f32" else None
        want = "f64" if r is None else "f32"
        if want != self.twin_values:
            self.invalidate_packed()
            self.twin_values = want
        return self if r is None else DeviceCSR(self.rowptr, self.colidx, r, self.shape)

    def cycle_source(self):
        """The matrix the twins stand for, as plain CSR: self, or -- twins that hold A32 -- a twinless view of A32 that
        shares the index arrays (built on demand: the inverse diagonals and the formats that do not narrow are taken from
        it, so that they agree with what the sweeps read)."""
        if self.twin_values == "f64":
            return self
        r = self._rounded()
        if r is None:
            raise LmgError("the values no longer fit fp32: call repack_values() after changing the values of a matrix")
        return DeviceCSR(self.rowptr, self.colidx, r, self.shape)

    def plain(self):
        """A twinless view of the same arrays: the sweeps on it run the plain CSR kernels on the fp64 values."""
        return DeviceCSR(self.rowptr, self.colidx, self.vals, self.shape)

    def repack_values(self):
        """After the values changed in place: refresh the twins (cheaply if possible) at the width pack() was asked for.
        Where the new values fail the range rule of the fp32 twins the matrix gets fp64 twins, and fp32 twins again once
        later values pass it."""
        had = any(t is not None for t in (self.patterns, self.sell, self.dia, self.packed))
        src = self._retarget() if self.values == "f32" else self
        if had and not any(t is not None for t in (self.patterns, self.sell, self.dia, self.packed)):
            self.pack()                                    # the twins changed kind: from scratch
            return
        if self.patterns is not None:
            self.patterns = RowPatterns.from_csr(src, self.patterns.grid_map)
            self._derive_grid_twins()
            if self.patterns is None:
                self.pack()
        if self.sell is not None and not self.sell.update_values(self):
            # update_values refused (fp32 values out of range): that twin again -- its columns, its padding -- in fp64
            self.sell = SellCSR.from_csr(self, colmode=self.sell.colmode, max_padding=float("inf"))
        if self.dia is not None and not self.dia.update_values(self):
            self.dia = None
        if self.packed is not None and not self.packed.update_values(src):
            self.packed = None
            self.pack(patterns=False)

    @classmethod
    def from_scipy(cls, A, device, canonical=True):
        """Any scipy.sparse matrix / ndarray -> sorted, duplicate-free CSR on `device`
        (the form pyamg hands its kernel after the CSC->CSR conversion, Multigrid.py:88)."""
        import scipy.sparse as sp
        if not (sp.isspmatrix_csr(A) and A.dtype == np.float64):
            A = sp.csr_matrix(A, dtype=np.float64)
        if canonical and not A.has_canonical_format:          # (SciPy caches the answer on the matrix object)
            A = A.copy()
            A.sum_duplicates()
        if A.nnz >= 2 ** 31 - 8192 or max(A.shape) >= 2 ** 31 - 1:
            raise ValueError("matrix too large for int32 indices")
        # (no host copies: SciPy holds int32 indices at these sizes already)
        return cls(torch.from_numpy(np.ascontiguousarray(A.indptr, dtype=np.int32)).to(device),
                   torch.from_numpy(np.ascontiguousarray(A.indices, dtype=np.int32)).to(device),
                   torch.from_numpy(np.ascontiguousarray(A.data, dtype=np.float64)).to(device), A.shape)

    def transpose(self):
        """A^T as a sorted CSR on the same device (setup: R = P^T).  A stable sort by column
        keeps the row order inside every column, i.e. the result is what SciPy's
        `A.T.tocsr()` gives for a canonical A."""
        n, m = self.shape
        dev = self.vals.device
        if self.vals.is_cuda and self.nnz and self.nnz < 2 ** 31 - 1:
            # counting sort on the column indices (csrc/transpose.hip): no library sort, whose code takes
            # 0.3 s to load in a fresh process
            L = _lib.lib()
            counts = torch.zeros(m, dtype=I32, device=dev)
            check(L.lmg_csr_transpose_count(self.nnz, m, _p(self.colidx), _p(counts), _s(self.colidx)), "lmg_csr_transpose_count")
            if int(counts.max()) <= int(L.lmg_csr_transpose_max_row()):
                rp = torch.empty(m + 1, dtype=I32, device=dev)
                exclusive_scan_i32(counts, rp)
                counts.zero_()
                tc = torch.empty(self.nnz, dtype=I32, device=dev)
                tv = torch.empty(self.nnz, dtype=F64, device=dev)
                check(L.lmg_csr_transpose_fill(n, m, _p(self.rowptr), _p(self.colidx), _p(self.vals), _p(rp), _p(counts),
                                               _p(tc), _p(tv), _s(self.rowptr)), "lmg_csr_transpose_fill")
                return DeviceCSR(rp, tc, tv, (m, n))
        rows = torch.repeat_interleave(torch.arange(n, device=dev, dtype=I32),
                                       (self.rowptr[1:] - self.rowptr[:-1]).long())
        order = torch.sort(self.colidx, stable=True).indices
        rp = torch.zeros(m + 1, dtype=I32, device=dev)
        if self.nnz:
            rp[1:] = torch.cumsum(torch.bincount(self.colidx, minlength=m), 0).to(I32)
        return DeviceCSR(rp, rows[order].contiguous(), self.vals[order].contiguous(), (m, n))

    def to_scipy(self):
        import scipy.sparse as sp
        return sp.csr_matrix((self.vals.cpu().numpy(), self.colidx.cpu().numpy(),
                              self.rowptr.cpu().numpy()), shape=self.shape)

    @property
    def device(self):
        return self.vals.device

    def bytes(self):
        return 12 * self.nnz + 4 * (self.shape[0] + 1)


_PACKED_ENABLED = True
_PATTERNS_ENABLED = True
_STENCIL_ENABLED = True
_GRID_MAPS_ENABLED = True
_DIA_ENABLED = True


def set_dia_enabled(flag):
    """Whether pack() builds the DIA twin of variable-coefficient grid operators (default), i.e. whether their
    smoothing steps run as fused passes (lmg_dia_smooth) or one launch per sweep (A/B runs and parity tests)."""
    global _DIA_ENABLED
    _DIA_ENABLED = bool(flag)


def set_grid_maps_enabled(flag):
    """Whether pack() tries row patterns with a column-base map on rectangular operators (default)."""
    global _GRID_MAPS_ENABLED
    _GRID_MAPS_ENABLED = bool(flag)


def set_stencil_enabled(flag):
    """Whether 3x3-stencil row-pattern matrices run lmg_stencil_sweep (default) or lmg_rpat_sweep."""
    global _STENCIL_ENABLED
    _STENCIL_ENABLED = bool(flag)


FUSED_MAX_SWEEPS = 3
# Two fused smoothing passes exist.  Levels beyond the Infinity Cache run the register-blocked pass of
# stencil_fused.hip (a wave marches down a strip of lines with all iterates in registers: least traffic, but every
# wave walks >= 12 lines one after the other); everything below runs the LDS-tiled pass of stencil_tile.hip (a
# workgroup per 64 x 16 tile, four waves per sweep).  Measured (tools/time_mid.py, 3 sweeps + residual / 3 sweeps,
# us): 9-point 2049^2 tile 71 / 54, register 97 / 61, separate 87 / 67; 5-point 2049^2 64 / 50, 67 / 44, 79 / 60;
# 5-point 1449^2 37 / 28, 59 / 37, 46 / 35; 4097^2: register 166 / 125, separate 300 / 226.  In the cfg#4 cycle
# the 2049^2 level on the tiled pass: 0.788 -> 0.766 ms.  The crossover lies between 9.4 M rows (5-point 3073^2: cycle 0.448 ms tiled,
# 0.459 register) and 16.8 M (5-point 4097^2: 0.65 vs 0.77; 9-point: 1.905 vs 1.913 at 8193^2 / 7 levels, i.e. equal).
FUSED_MIN_ROWS = 12_000_000
REG_MAX_ROWS = (1 << 29) - 4096      # lmg_stencil_smooth* (32-bit byte offsets); lmg_stencil_gs_sweep: (1 << 29) - 8192
GS_WAVE_MAX_ROWS = (1 << 29) - 8192
# The tiled pass takes over below, down to levels that are a handful of workgroups either way.
TILED_MIN_ROWS = 4096
_TILED_ENABLED = True


def set_tiled_enabled(flag):
    """Whether small grid-stencil levels run their sweeps as LDS-tiled fused passes (default) or one launch per
    sweep (A/B runs and parity tests)."""
    global _TILED_ENABLED
    _TILED_ENABLED = bool(flag)


def _pass_kind(A, cheby):
    """'reg' (stencil_fused.hip), 'tile' (stencil_tile.hip), 'dia' (dia_tile.hip: per-row values) or None: how a
    smoothing step -- Jacobi sweeps, or with `cheby` a Chebyshev step -- would run on A as one pass."""
    S = getattr(A, "stencil", None)
    D = getattr(A, "dia", None)
    if S is None and D is not None and _PACKED_ENABLED and _DIA_ENABLED and _FUSED_ENABLED:
        return "dia"
    if not (_PACKED_ENABLED and _STENCIL_ENABLED and _FUSED_ENABLED and S is not None):
        return None
    if S.n >= FUSED_MIN_ROWS and not cheby:
        # (the register pass addresses with 32-bit byte offsets: beyond REG_MAX_ROWS the separate sweeps run)
        return "reg" if (S.n < REG_MAX_ROWS and _lib.lib().lmg_stencil_smooth_supported(S.umask)) else None
    # the register pass has no Chebyshev form: a Chebyshev step stays on the tiled pass, up to CHEBY_TILED_MAX_ROWS rows
    if (_TILED_ENABLED and S.n >= TILED_MIN_ROWS and not (cheby and S.n > CHEBY_TILED_MAX_ROWS) and S.W >= 3
            and _lib.lib().lmg_stencil_smooth_tiled_supported(S.umask)):
        return "tile"
    return None


def _fused_kind(A):
    """How stencil_smooth would run on A (_pass_kind)."""
    return _pass_kind(A, False)


def stencil_smooth_available(A):
    """True when `A` has a grid-stencil twin whose smoothing passes stencil_smooth can run fused."""
    return _fused_kind(A) is not None


_FUSED_ENABLED = True


def set_fused_enabled(flag):
    """Whether Hierarchy.smooth may fuse the Jacobi sweeps of a level visit (default) or launches them
    one by one (A/B runs and parity tests)."""
    global _FUSED_ENABLED
    _FUSED_ENABLED = bool(flag)


def stencil_smooth(A, x_in, b, omega, sweeps, x_out, r_out=None, prolong=None, restrict=None):
    """x_out = `sweeps` (1..3) weighted-Jacobi sweeps from x_in (None = zero iterate), r_out = b - A x_out
    (optional), in one pass (lmg_stencil_smooth); same bits as the separate csr_jacobi / vmul /
    csr_residual_norm2 launches.  prolong = (P, e): the sweeps start from x_in + P e (the correction of
    Multigrid.py:115, never written: lmg_stencil_smooth_prolong; see stencil_smooth_prolong_available).
    restrict = (R, b_coarse): b_coarse = R (b - A x_out) instead of r_out (Multigrid.py:90 + :93, the residual is
    never written: lmg_stencil_smooth_restrict; see stencil_smooth_restrict_available)."""
    _vec_ok(x_in, b, x_out, r_out)
    if A.stencil is not None:
        kind = "tile" if _fused_kind(A) == "tile" else "reg"
    elif getattr(A, "dia", None) is not None:
        kind = "dia"
    else:
        raise LmgError("stencil_smooth needs a grid-stencil matrix")
    _run_pass("smooth", kind, A, (int(sweeps), _p(x_in), _p(b), float(omega), _p(x_out)), x_in, r_out, prolong, restrict)


def _run_pass(stem, kind, A, head, x_in, r_out, prolong, restrict):
    """The call of stencil_smooth (stem "smooth") and stencil_cheby ("cheby") on a level that runs the pass `kind`:
    lmg_dia_<stem> or lmg_stencil_<stem>[_tiled][_prolong | _restrict].  head: the C arguments from the sweep count to
    x_out."""
    who = "stencil_" + stem
    if kind == "dia":
        D = A.dia
        if prolong is not None or restrict is not None:
            raise LmgError("%s: transfers cannot be fused into the pass of a variable-coefficient operator" % who)
        name = "lmg_dia_" + stem + ("_f32" if D.values == "f32" else "")
        check(getattr(_lib.lib(), name)(D.n, D.W, D.umask, _p(D.dia), *head, _p(r_out), _s(D.dia)), name)
        return
    S = A.stencil
    tiled = kind == "tile"
    form = "restrict" if restrict is not None else "prolong" if prolong is not None else None
    if form is None:
        tail = (_p(r_out),)
    else:
        M, vec = restrict if form == "restrict" else prolong
        T = getattr(M, form)
        _vec_ok(vec)
        # the restricting pass takes no correction, the correcting pass no zero iterate
        other = prolong is not None if form == "restrict" else x_in is None
        if T is None or r_out is not None or other or T.n != S.n or T.W != S.W or vec.numel() != T.nc:
            what = "restriction" if form == "restrict" else "prolongation"
            raise LmgError("%s: this %s cannot be fused into the pass" % (who, what))
        # Jacobi only: a level on the tiled passes may take the register pass for this launch (A/B knobs)
        reg_min = REG_RESTRICT_MIN_ROWS if form == "restrict" else REG_PROLONG_MIN_ROWS
        if (stem == "smooth" and S.n >= reg_min and _lib.lib().lmg_stencil_smooth_prolong_supported(S.umask)
                and not S.line_end_coupling):
            tiled = False
        if not tiled and S.line_end_coupling:
            # (the register pass finds the coarse window of an element by its lane: wrong for the elements beyond a line end,
            # which only such an operator reads -- include/lmg.h; the tiled pass finds it by the element's own line and column)
            raise LmgError("%s: the register pass folds no transfer into an operator with entries across a line end" % who)
        tail = T.c_args(vec)
    name = "lmg_stencil_%s%s%s" % (stem, "_tiled" if tiled else "", "_" + form if form else "")
    if not tiled and stem == "smooth" and _FUSED_UNIFORM_ENABLED and S.census is not None:
        # the register pass with the census tables of the twins: waves that meet only hot rows never look at an id
        name += "_census"
        tail += _census_args(S, T if form else None, form)
    check(getattr(_lib.lib(), name)(*S.c_args(), *head, *tail, _s(S.pid)), name)


_FUSED_UNIFORM_ENABLED = True


def set_fused_uniform_enabled(flag):
    """Whether the register-fused passes are handed the census tables of their twins (default), i.e. whether waves that
    read nothing but hot rows run the id-free body, or every launch goes to the entry points without tables (A/B runs
    and parity tests).  Same bits either way."""
    global _FUSED_UNIFORM_ENABLED
    _FUSED_UNIFORM_ENABLED = bool(flag)


def _census_args(S, T, form):
    """The trailing arguments of lmg_stencil_smooth[_prolong | _restrict]_census: the tables of the operator's twin S and
    of the transfer's twin T (None where a twin has none) and their row strides."""
    if form is None:
        return (_p(S.census), census_stride(S.W))
    if form == "prolong":
        return (_p(S.census), _p(T.census), census_stride(S.W))
    return (_p(S.census), census_stride(S.W), _p(T.census), census_stride(T.Wc))


def fused_uniform_items(A, sweeps, with_residual=False, zero=False, prolong=None, restrict=None):
    """(general, fast, uniform): how many items (waves) of the register-fused pass that stencil_smooth would launch on A
    with these arguments run each body -- the kernel's own predicate, evaluated on the host from copies of the census
    tables (lmg_stencil_smooth_uniform_items), with the tune keys as they stand.  prolong / restrict: the transfer
    matrix whose twin the pass folds in.  Twins without a table count as the kernel sees them: no uniform item."""
    S = A.stencil
    form, T = (1, prolong.prolong) if prolong is not None else (2, restrict.restrict) if restrict is not None else (0, None)
    use = _FUSED_UNIFORM_ENABLED
    host = [None if (t is None or not use) else t.cpu().numpy() for t in
            (S.census, T.census if form == 1 else None, T.census if form == 2 else None)]
    counts = (ctypes.c_int64 * 3)()
    check(_lib.lib().lmg_stencil_smooth_uniform_items(
        S.n, S.W, int(sweeps), int(bool(with_residual or form == 2)), int(bool(zero)), form, T.nc if T is not None else 0,
        T.Wc if T is not None else 0, *[None if h is None else h.ctypes.data for h in host], ctypes.addressof(counts)),
        "lmg_stencil_smooth_uniform_items")
    return tuple(int(c) for c in counts)


# The transfers are folded into the fused passes only on levels that do not fit the Infinity Cache: what is saved is
# HBM traffic (the residual / the corrected iterate are never written and re-read); on a cache-resident level the
# passes are bound by their arithmetic and the extra work costs more than the two small launches it replaces
# (measured in the cycle, cfg#4: 4097^2 5-point -52 us and -7 us, 2049^2 9-point +8 us and +4 us).
FUSED_TRANSFER_MIN_ROWS = 12_000_000
# Levels that run the tiled passes may still take the REGISTER pass for the launch with the correction / the restriction
# folded in from this many rows on (A/B knobs; see DESIGN.md section 4 for what was measured).
REG_PROLONG_MIN_ROWS = 1 << 62
REG_RESTRICT_MIN_ROWS = 1 << 62
_FUSED_PROLONG_ENABLED = True


def set_fused_prolong_enabled(flag):
    """Whether the coarse-grid correction may be folded into the fused post-smoothing pass (default) or runs as
    its own launch (A/B runs and parity tests)."""
    global _FUSED_PROLONG_ENABLED
    _FUSED_PROLONG_ENABLED = bool(flag)


def _twin_on_grid(A, M, form):
    """The grid twin of transfer M (form "prolong" or "restrict") where it sits on the grid of A's stencil twin, else None."""
    T = getattr(M, form, None)
    S = getattr(A, "stencil", None)
    return T if (T is not None and S is not None and T.n == S.n and T.W == S.W) else None


def _prolong_available(A, P, kind):
    if not (_FUSED_PROLONG_ENABLED and kind in ("reg", "tile") and _twin_on_grid(A, P, "prolong") is not None):
        return False
    if kind == "tile":                   # the tile is loaded as x + P e: always cheaper than the P launch it replaces
        return True
    S = A.stencil
    return bool(S.n >= FUSED_TRANSFER_MIN_ROWS and _lib.lib().lmg_stencil_smooth_prolong_supported(S.umask)
                and not S.line_end_coupling)


def stencil_smooth_prolong_available(A, P):
    """True when stencil_smooth can take `prolong=(P, e)`: A runs fused passes and P is a 2x2-window grid
    prolongation onto A's grid."""
    return _prolong_available(A, P, _fused_kind(A))


_FUSED_RESTRICT_ENABLED = True
# The tiled pass may fold the restriction in up to this many rows: it costs one more halo line / column per tile.  With
# 16-line tiles that was a loss from 4 M rows on (30 % more arithmetic); with 32-line tiles it pays on every tiled level
# (cfg#4 cycle 0.652 vs 0.654 ms with the 2049^2 level excluded, 0.661 without any; cfg#2 0.151 vs 0.157 ms).
TILED_RESTRICT_MAX_ROWS = 1 << 62


def set_fused_restrict_enabled(flag):
    """Whether the restriction of the residual may be folded into the fused pre-smoothing pass (default) or the
    residual is stored and restricted by its own launch (A/B runs and parity tests)."""
    global _FUSED_RESTRICT_ENABLED
    _FUSED_RESTRICT_ENABLED = bool(flag)


def _restrict_available(A, R, kind):
    T = _twin_on_grid(A, R, "restrict")
    if not (_FUSED_RESTRICT_ENABLED and kind in ("reg", "tile") and T is not None):
        return False
    S = A.stencil
    if kind == "reg" and not (S.n >= FUSED_TRANSFER_MIN_ROWS and _lib.lib().lmg_stencil_smooth_prolong_supported(S.umask)
                              and not S.line_end_coupling):
        return False
    if kind == "tile" and S.n > TILED_RESTRICT_MAX_ROWS:
        return False
    lines = (S.n + S.W - 1) // S.W
    return T.nc >= ((lines + 1) // 2 - 1) * T.Wc + (S.W + 1) // 2


def stencil_smooth_restrict_available(A, R):
    """True when stencil_smooth can take `restrict=(R, b_coarse)`: A runs fused passes and R is the 3x3-window
    restriction from A's grid with a coarse row under every (even line, even column) node."""
    return _restrict_available(A, R, _fused_kind(A))


_FUSED_TURNAROUND_ENABLED = True
# The hierarchy runs the turnaround of a repeated visit (W- and F-cycles) as one pass on levels of TURNAROUND_MIN_ROWS to
# TURNAROUND_MAX_ROWS rows and keeps the correcting and the restricting pass elsewhere.  Measured at 3 + 3 sweeps, 9-point
# Galerkin levels of cfg#4 (tools/time_cycle_shapes.py, us per pair, two passes / one pass): 2049^2 108.7 / 121.9 (64-line
# tiles; 134.0 with 32), 1025^2 43.3 / 41.7 (64), 513^2 21.5 / 19.8 (32), 257^2 14.6 / 14.8 (32): the extra halo work
# loses where the passes are instruction-bound and only pays on the latency-bound middle levels.
TURNAROUND_MIN_ROWS = 100_000
TURNAROUND_MAX_ROWS = 2_000_000


def set_fused_turnaround_enabled(flag):
    """Whether the turnaround of a repeated level visit -- the post-smoothing pass of visit k, the pre-smoothing pass
    of visit k + 1 -- may run as one pass (default) or as the correcting and the restricting pass (A/B runs and
    parity tests)."""
    global _FUSED_TURNAROUND_ENABLED
    _FUSED_TURNAROUND_ENABLED = bool(flag)


def stencil_smooth_turnaround_available(A, P, R):
    """True when stencil_smooth_turnaround can run on level operator A with prolongation P and restriction R: A runs
    the tiled passes, both transfers fold into them and share one coarse grid."""
    if not (_FUSED_TURNAROUND_ENABLED and _fused_kind(A) == "tile"):
        return False
    if not (stencil_smooth_prolong_available(A, P) and stencil_smooth_restrict_available(A, R)):
        return False
    S, TP, TR = A.stencil, P.prolong, R.restrict
    lines = (S.n + S.W - 1) // S.W
    return bool(TP.nc == TR.nc and TP.Wc == TR.Wc and TR.nc >= 2 and S.n % S.W == 0
                and TR.Wc == (S.W + 1) // 2 and TR.nc == ((lines + 1) // 2) * TR.Wc)


def stencil_smooth_turnaround_selected(A, P, R):
    """True where the hierarchy runs the turnaround pass: available, and the level's size is one where it was measured
    to beat the two passes (TURNAROUND_MIN_ROWS .. TURNAROUND_MAX_ROWS)."""
    return bool(stencil_smooth_turnaround_available(A, P, R) and TURNAROUND_MIN_ROWS <= A.shape[0] <= TURNAROUND_MAX_ROWS)


def stencil_smooth_turnaround(A, x_in, b, omega, sweeps_post, sweeps_pre, x_out, prolong, restrict):
    """x_out = J^(sweeps_post + sweeps_pre)(x_in + P e), b_coarse = R (b - A x_out) in ONE tiled pass
    (lmg_stencil_smooth_tiled_turnaround): the post-smoothing pass of one visit of a level and the pre-smoothing pass of
    the next visit, as W- and F-cycles repeat them.  prolong = (P, e), restrict = (R, b_coarse); sweeps 1..3 each.
    Same bits as stencil_smooth(..., prolong=(P, e)) followed by stencil_smooth(..., restrict=(R, b_coarse))."""
    (P, e), (R, bc) = prolong, restrict
    _vec_ok(x_in, b, x_out, e, bc)
    S, TP, TR = A.stencil, getattr(P, "prolong", None), getattr(R, "restrict", None)
    if (S is None or TP is None or TR is None or x_in is None or _fused_kind(A) != "tile" or TP.n != S.n or TP.W != S.W
            or TR.n != S.n or TR.W != S.W or e.numel() != TP.nc or bc.numel() != TR.nc):
        raise LmgError("stencil_smooth_turnaround: this level and its transfers cannot run the turnaround pass")
    check(_lib.lib().lmg_stencil_smooth_tiled_turnaround(
        *S.c_args(), int(sweeps_post), int(sweeps_pre), _p(x_in), _p(b), float(omega), _p(x_out), *TP.c_args(e),
        *TR.c_args(bc)[2:], _s(S.pid)), "lmg_stencil_smooth_tiled_turnaround")


# ---- Chebyshev polynomial smoother (hierarchy.py: smoother="Chebyshev") -------------------------------------------------
# One smoothing step of degree S is S sweeps d = a_k d + c_k D^-1 (b - A x), x += d; `coef` = [(a_0, c_0), ...] is the
# host's table (hierarchy.chebyshev_coefficients).  Levels with a stencil or DIA twin run a step of degree <= 3 as ONE tiled
# pass (lmg_stencil_cheby_tiled*, lmg_dia_cheby), every other format -- and every degree above 3 -- as the residual launch
# plus cheby_update per sweep.  The register-marching pass has no Chebyshev variant: levels from FUSED_MIN_ROWS rows on
# run the tiled pass too, up to CHEBY_TILED_MAX_ROWS rows (the two-launch path beyond; see DESIGN.md for the 4097^2 times).
CHEBY_TILED_MAX_ROWS = (1 << 31) - 4096 - 1


def _cheby_kind(A):
    """'tile' (stencil_tile.hip), 'dia' (dia_tile.hip) or None: how stencil_cheby would run on A (_pass_kind)."""
    return _pass_kind(A, True)


def stencil_cheby_available(A):
    """True when `A` has a stencil or DIA twin on which stencil_cheby runs a Chebyshev step as one pass."""
    return _cheby_kind(A) is not None


def stencil_cheby_prolong_available(A, P):
    """True when stencil_cheby can take `prolong=(P, e)` (the rule of the tiled Jacobi pass: always where it can)."""
    return _prolong_available(A, P, _cheby_kind(A))


def stencil_cheby_restrict_available(A, R):
    """True when stencil_cheby can take `restrict=(R, b_coarse)` (the rule of the tiled Jacobi pass)."""
    return _restrict_available(A, R, _cheby_kind(A))


def _cheby_coef(coef):
    flat = [float(v) for pair in coef for v in pair]
    if not 1 <= len(coef) <= FUSED_MAX_SWEEPS or len(flat) != 2 * len(coef):
        raise LmgError("stencil_cheby takes 1..%d (a_k, c_k) pairs, got %r" % (FUSED_MAX_SWEEPS, coef))
    return (ctypes.c_double * len(flat))(*flat)


def stencil_cheby(A, x_in, b, coef, x_out, r_out=None, prolong=None, restrict=None):
    """x_out = one Chebyshev step of degree len(coef) (1..3) from x_in (None = zero iterate), r_out = b - A x_out
    (optional), in one tiled pass; same bits as csr_residual_norm2 + cheby_update per sweep.  prolong = (P, e) and
    restrict = (R, b_coarse) as in stencil_smooth (stencil twins only; see stencil_cheby_*_available)."""
    _vec_ok(x_in, b, x_out, r_out)
    kind = _cheby_kind(A)
    hc = _cheby_coef(coef)
    if kind is None:
        raise LmgError("stencil_cheby needs a level that runs the tiled passes (stencil_cheby_available)")
    _run_pass("cheby", kind, A, (len(coef), ctypes.addressof(hc), _p(x_in), _p(b), _p(x_out)), x_in, r_out, prolong, restrict)


def cheby_update(a, c, dinv, r, d, x, first=False):
    """d = a * d + c * (dinv * r) (first: d = c * (dinv * r), d is not read); x += d -- the Chebyshev sweep after a
    residual launch (lmg_cheby_update)."""
    _vec_ok(dinv, r, d, x)
    check(_lib.lib().lmg_cheby_update(x.numel(), float(a), float(c), int(bool(first)), _p(dinv), _p(r), _p(d), _p(x), _s(x)),
          "lmg_cheby_update")


def csr_gershgorin(A, out):
    """out[0] = max_i (sum_j |a_ij|) / |a_ii|, the Gershgorin bound of the spectrum of D^-1 A (lmg_csr_gershgorin)."""
    _vec_ok(out)
    check(_lib.lib().lmg_csr_gershgorin(A.shape[0], _p(A.rowptr), _p(A.colidx), _p(A.vals), _p(out), _s(A.rowptr)),
          "lmg_csr_gershgorin")


# ---- line relaxation (csrc/line.hip) -------------------------------------------------------------------------------------
LINE_DIRS = {"x": 0, "y": 1}        # the `dir` of lmg_line_factor / lmg_line_solve
LINE_COUPLED, LINE_PIVOT = 1, 2     # the bits of their flag word


def line_factor_flags(A, W, dir):
    """((lo, minv, cp), flags): the factored tridiagonal systems of the grid lines of A in direction "x" | "y" for line
    stride W (lmg_line_factor: two launches, setup) and its flag word -- LINE_COUPLED: a non-zero entry couples two x-lines,
    LINE_PIVOT: a zero or non-finite pivot.  One 4-byte device -> host read: never while a hipGraph is being captured."""
    if dir not in LINE_DIRS:
        raise ValueError("line direction must be 'x' or 'y', got %r" % (dir,))
    n = A.shape[0]
    if A.shape[0] != A.shape[1] or int(W) < 1 or n % int(W) != 0:
        raise ValueError("line relaxation needs a square operator whose %d rows are whole lines of %r" % (n, W))
    dev = A.vals.device
    lo, minv, cp = (torch.empty(n, dtype=F64, device=dev) for _ in range(3))
    flags = torch.zeros(1, dtype=I32, device=dev)
    check(_lib.lib().lmg_line_factor(n, int(W), LINE_DIRS[dir], _p(A.rowptr), _p(A.colidx), _p(A.vals), _p(lo), _p(minv),
                                     _p(cp), _p(flags), _s(A.rowptr)), "lmg_line_factor")
    return (lo, minv, cp), int(flags.item())


def line_factor(A, W, dir):
    """The factor triple (lo, minv, cp) of line_factor_flags, or a ValueError that says which flag was set."""
    fac, flags = line_factor_flags(A, W, dir)
    if flags & LINE_COUPLED:
        raise ValueError("a non-zero entry couples two x-lines (an entry across the end of a line)")
    if flags & LINE_PIVOT:
        raise ValueError("a zero or non-finite pivot in the %s-line systems" % dir)
    return fac


def line_solve(W, dir, first, step, fac, r, omega, x):
    """x += omega * T^-1 r on the systems first, first + step, ... of direction dir; r (the residual, formed before the
    call) is overwritten on those systems, every other row of x and r keeps its bits (lmg_line_solve)."""
    lo, minv, cp = fac
    _vec_ok(lo, minv, cp, r, x)
    n = x.numel()
    if any(t.numel() != n for t in (lo, minv, cp, r)):
        raise ValueError("line_solve: the factors, r and x must have one entry per row")
    if dir not in LINE_DIRS:
        raise ValueError("line direction must be 'x' or 'y', got %r" % (dir,))
    check(_lib.lib().lmg_line_solve(n, int(W), LINE_DIRS[dir], int(first), int(step), _p(lo), _p(minv), _p(cp), _p(r),
                                    float(omega), _p(x), _s(x)), "lmg_line_solve")


LINE_SOLVE_BANDS = (2, 3)           # the half-bandwidths of lmg_line_factor_banded / lmg_line_solve_banded (1: the pair above)


def _line_band(band):
    if band not in LINE_SOLVE_BANDS or isinstance(band, bool):
        raise ValueError("the banded line kernels take band 2 or 3, got %r" % (band,))
    return int(band)


def line_factor_banded_flags(A, W, dir, band):
    """(fac, flags): the factored banded systems (half-bandwidth `band`, 2 | 3) of the grid lines of A in direction "x" | "y"
    for line stride W, and the flag word of line_factor_flags.  fac is one tensor of (2 band + 1) n doubles, 2 band + 1 planes
    indexed by row: `band` multipliers, minv, `band` upper entries (lmg_line_factor_banded: two launches, setup).  One
    4-byte device -> host read: never while a hipGraph is being captured."""
    if dir not in LINE_DIRS:
        raise ValueError("line direction must be 'x' or 'y', got %r" % (dir,))
    band = _line_band(band)
    n = A.shape[0]
    if A.shape[0] != A.shape[1] or int(W) < 1 or n % int(W) != 0:
        raise ValueError("line relaxation needs a square operator whose %d rows are whole lines of %r" % (n, W))
    dev = A.vals.device
    fac = torch.empty((2 * band + 1) * n, dtype=F64, device=dev)
    flags = torch.zeros(1, dtype=I32, device=dev)
    check(_lib.lib().lmg_line_factor_banded(n, int(W), LINE_DIRS[dir], band, _p(A.rowptr), _p(A.colidx), _p(A.vals), _p(fac),
                                            _p(flags), _s(A.rowptr)), "lmg_line_factor_banded")
    return fac, int(flags.item())


def line_factor_banded(A, W, dir, band):
    """The factors of line_factor_banded_flags, or a ValueError that says which flag was set."""
    fac, flags = line_factor_banded_flags(A, W, dir, band)
    if flags & LINE_COUPLED:
        raise ValueError("a non-zero entry couples two x-lines (an entry across the end of a line)")
    if flags & LINE_PIVOT:
        raise ValueError("a zero or non-finite pivot in the %s-line systems" % dir)
    return fac


def line_solve_banded(W, dir, band, first, step, fac, r, omega, x):
    """x += omega * (L U)^-1 r on the systems first, first + step, ... of direction dir, L U the banded factors `fac` of
    line_factor_banded; r (the residual, formed before the call) is overwritten on those systems, every other row of x and
    r keeps its bits (lmg_line_solve_banded)."""
    band = _line_band(band)
    _vec_ok(fac, r, x)
    n = x.numel()
    if r.numel() != n or fac.numel() != (2 * band + 1) * n:
        raise ValueError("line_solve_banded: r and x must have one entry per row, the factors %d" % (2 * band + 1))
    if dir not in LINE_DIRS:
        raise ValueError("line direction must be 'x' or 'y', got %r" % (dir,))
    check(_lib.lib().lmg_line_solve_banded(n, int(W), LINE_DIRS[dir], band, int(first), int(step), _p(fac), _p(r),
                                           float(omega), _p(x), _s(x)), "lmg_line_solve_banded")


def _use_stencil(A, *vecs):
    if not (_PACKED_ENABLED and _STENCIL_ENABLED and A.stencil is not None):
        return False
    return all(v is None or v.data_ptr() % 16 == 0 for v in vecs)


_SELL_ENABLED = True
SELL_MIN_AVG = 12.0          # average row length from which the sliced-ELL twin replaces the packed CSR


def set_sell_enabled(flag):
    """Whether pack() may pick the sliced-ELL twin for long rows (default) or keeps the packed CSR."""
    global _SELL_ENABLED
    _SELL_ENABLED = bool(flag)


def set_packed_enabled(flag):
    """Route csr_jacobi / csr_residual_norm2 / csr_spmv through the lossless twins when they
    exist (default) or always through the plain CSR kernels (A/B and parity tests)."""
    global _PACKED_ENABLED
    _PACKED_ENABLED = bool(flag)


def set_patterns_enabled(flag):
    """Whether pack() may pick the row-pattern twin (default) or always builds the packed CSR."""
    global _PATTERNS_ENABLED
    _PATTERNS_ENABLED = bool(flag)


def partials_count(n):
    return int(_lib.lib().lmg_partials_count(int(n)))


def tune_set(key, value):
    check(_lib.lib().lmg_tune_set(key.encode(), int(value)), "lmg_tune_set")


def tune_get(key):
    return check(_lib.lib().lmg_tune_get(key.encode()), "lmg_tune_get")


# ---- sweeps ------------------------------------------------------------------------
_MODE_NAMES = ("residual", "jacobi", "spmv")


def _twin_sweep(entry, mode, twin, tail):
    """entry = the lmg_*_sweep function of the twin's format; tail: the vectors and scalars every one of them ends with."""
    head, t = twin.sweep_args()
    return entry(mode, *head, *tail, _s(t))


def _sweep(mode, A, x, b, out, alpha, beta, partials, norm2):
    """One sweep (0 residual, 1 Jacobi, 2 SpMV) on the best twin A has: grid stencil -> row patterns -> sliced ELL ->
    packed CSR -> plain CSR."""
    what = "(%s)" % _MODE_NAMES[mode]
    L = _lib.lib()
    tail = (_p(x), _p(b), _p(out), float(alpha), float(beta), _p(partials), _p(norm2))
    if _use_stencil(A, x, b, out):
        check(_twin_sweep(L.lmg_stencil_sweep, mode, A.stencil, tail), "lmg_stencil_sweep" + what)
        return
    if _PACKED_ENABLED and A.patterns is not None:
        check(_twin_sweep(L.lmg_rpat_sweep_grid, mode, A.patterns, tail), "lmg_rpat_sweep" + what)
        return
    if _PACKED_ENABLED and A.sell is not None:
        name = "lmg_sell_sweep_f32" if A.sell.values == "f32" else "lmg_sell_sweep"
        check(_twin_sweep(getattr(L, name), mode, A.sell, tail), name + what)
        return
    if _PACKED_ENABLED and A.packed is not None:
        rc = _twin_sweep(L.lmg_pcsr_sweep, mode, A.packed, tail)
        if rc != -4:                                   # LMG_ERR_CAPACITY: tile too large for LDS
            check(rc, "lmg_pcsr_sweep" + what)
            return
    csr = (A.shape[0], A.nnz, _p(A.rowptr), _p(A.colidx), _p(A.vals))
    if mode == 0:
        check(L.lmg_csr_residual_norm2(*csr, _p(x), _p(b), _p(out), _p(partials), _p(norm2), _s(A.rowptr)),
              "lmg_csr_residual_norm2")
    elif mode == 1:
        check(L.lmg_csr_jacobi(*csr, _p(x), _p(b), float(alpha), _p(out), _s(A.rowptr)), "lmg_csr_jacobi")
    else:
        check(L.lmg_csr_spmv(*csr, _p(x), _p(out), float(alpha), float(beta), _s(A.rowptr)), "lmg_csr_spmv")


def csr_residual_norm2(A, x, b, r, partials, norm2):
    """r = b - A x (r may be None), norm2[0] = sum r_i^2 (partials/norm2 may both be None)."""
    _vec_ok(x, b, r, partials, norm2)
    _sweep(0, A, x, b, r, 0.0, 0.0, partials, norm2)


def csr_jacobi(A, x_in, b, omega, x_out):
    _vec_ok(x_in, b, x_out)
    _sweep(1, A, x_in, b, x_out, omega, 0.0, None, None)


def csr_spmv(A, x, y, alpha=1.0, beta=0.0):
    _vec_ok(x, y)
    if x.numel() != A.shape[1] or y.numel() != A.shape[0]:
        raise ValueError("spmv shape mismatch: A %s, x %d, y %d" % (A.shape, x.numel(), y.numel()))
    _sweep(2, A, x, None, y, alpha, beta, None, None)


# ---- sweeps on a block of right-hand sides ---------------------------------------------------------
# A block of k vectors is a 2-D contiguous (n, k) tensor -- X[i, j] at i * k + j --, k in BLOCK_WIDTHS, 16-byte aligned: the
# matrix bytes of a sweep are read once for the k columns (lmg_sell_sweep_block), column j with the bits of the
# single-vector SELL sweep on column j.  The driver is block.py (BlockCycle); nothing here is a torch.ops.lmg op.
BLOCK_WIDTHS = (2, 4, 8)


def block_twin(A):
    """The fp64 sliced-ELL twin the block sweeps read, of any DeviceCSR (square or rectangular): A.sell where pack() chose
    one with fp64 values, else a twin of its own, built whatever the padding costs."""
    S = A.sell
    if S is None or S.values != "f64":
        S = SellCSR.from_csr(A, max_padding=float("inf"))
    if S is None:
        raise ValueError("block_twin: a %s matrix with %d entries has no sliced-ELL twin" % (A.shape, A.nnz))
    return S


def _block_ok(*blocks):
    """2-D contiguous float64 device tensors (rows, k) of one width k in BLOCK_WIDTHS, 16-byte aligned; returns k."""
    k = None
    for t in blocks:
        if t is None:
            continue
        _vec_ok(t)
        if t.dim() != 2 or t.shape[1] not in BLOCK_WIDTHS or t.shape[1] != (k or t.shape[1]):
            raise ValueError("expected (rows, k) blocks of one width k in %s, got %s" % (BLOCK_WIDTHS, tuple(t.shape)))
        if t.data_ptr() % 16:
            raise ValueError("a block must start at a 16-byte aligned address")
        k = t.shape[1]
    return k


def _block_sweep(mode, S, X, B, Out, alpha, beta, partials, norm2):
    k = _block_ok(X, B, Out)
    n, m = S.shape
    if X.shape[0] != m or any(t is not None and t.shape[0] != n for t in (B, Out)):
        raise ValueError("block %s: matrix %s, X %s, B %s, Out %s" % (_MODE_NAMES[mode], S.shape, tuple(X.shape),
                                                                       None if B is None else tuple(B.shape),
                                                                       None if Out is None else tuple(Out.shape)))
    if S.values != "f64":
        raise ValueError("the block sweeps read fp64 values: build the twin with block_twin()")
    head, t = S.sweep_args()
    check(_lib.lib().lmg_sell_sweep_block(mode, k, *head, _p(X), _p(B), _p(Out), float(alpha), float(beta), _p(partials),
                                          _p(norm2), _s(t)), "lmg_sell_sweep_block(%s)" % _MODE_NAMES[mode])


def block_partials_count(n, k):
    return int(_lib.lib().lmg_block_partials_count(int(n), int(k)))


def block_residual_norm2(S, X, B, R, partials, norm2):
    """R = B - A X (R may be None), norm2[j] = sum_i R[i, j]^2 for the k columns (partials / norm2 may both be None)."""
    _vec_ok(partials, norm2)
    k = _block_ok(X)
    if (partials is None) != (norm2 is None):
        raise ValueError("block_residual_norm2: partials and norm2 come together")
    if norm2 is not None and (norm2.numel() < k or partials.numel() < block_partials_count(S.n, k)):
        raise ValueError("block_residual_norm2: norm2 or partials too short for %d columns" % k)
    if S.shape[0] != S.shape[1]:
        raise ValueError("block_residual_norm2 needs a square matrix, got %s" % (S.shape,))
    _block_sweep(0, S, X, B, R, 0.0, 0.0, partials, norm2)


def block_jacobi(S, X, B, omega, Out):
    """Out = X + omega D^-1 (B - A X) column by column (rows without a diagonal keep X); Out must not overlap X."""
    if S.shape[0] != S.shape[1]:
        raise ValueError("block_jacobi needs a square matrix, got %s" % (S.shape,))
    _block_sweep(1, S, X, B, Out, omega, 0.0, None, None)


def block_spmv(S, X, Y, alpha=1.0, beta=0.0):
    """Y = alpha A X + beta Y column by column; Y must not overlap X."""
    _block_sweep(2, S, X, None, Y, alpha, beta, None, None)


def block_dot_partials_count(n, k):
    return int(_lib.lib().lmg_block_dot_partials_count(int(n), int(k)))


def _block_scalars_ok(k, *scalars):
    """Per-column scalars: contiguous float64 device tensors of at least k elements."""
    _vec_ok(*scalars)
    if any(t.numel() < k for t in scalars):
        raise ValueError("a per-column scalar array is shorter than the %d columns of the block" % k)


def _block_same_shape(name, *blocks):
    k = _block_ok(*blocks)
    if any(t.shape != blocks[0].shape for t in blocks):
        raise ValueError("%s: blocks of different shapes %s" % (name, [tuple(t.shape) for t in blocks]))
    return k


def block_dot(X, Y, partials, out):
    """out[j] = X[:, j] . Y[:, j] for the k columns in one pass; column j has the bits of dot() on a contiguous column j."""
    k = _block_same_shape("block_dot", X, Y)
    _block_scalars_ok(k, out)
    _vec_ok(partials)
    if partials.numel() < block_dot_partials_count(X.shape[0], k):
        raise ValueError("block_dot: partials too short for %d columns" % k)
    check(_lib.lib().lmg_block_dot(k, X.shape[0], _p(X), _p(Y), _p(partials), _p(out), _s(X)), "lmg_block_dot")


def block_cg_step(rz, pAp, tol2, mask, P, AP, X, R, partials, rr):
    """The fused update of a CG iteration on a block, all scalars on the device: alpha_j = rz[j] / pAp[j] (0 where mask[j] or
    pAp[j] is 0), X += alpha P and R -= alpha AP for the columns with mask[j] != 0 -- the bits of axpby(alpha, p, 1, x) and
    axpby(-alpha, ap, 1, r); the other columns of X and R are not stored --, rr[j] = |R[:, j]|^2 with block_dot's bits, and
    mask[j] = 1.0 if mask[j] != 0 and rr[j] > tol2[j] else 0.0."""
    k = _block_same_shape("block_cg_step", P, AP, X, R)
    _block_scalars_ok(k, rz, pAp, tol2, mask, rr)
    _vec_ok(partials)
    if partials.numel() < block_dot_partials_count(X.shape[0], k):
        raise ValueError("block_cg_step: partials too short for %d columns" % k)
    check(_lib.lib().lmg_block_cg_step(k, X.shape[0], _p(rz), _p(pAp), _p(tol2), _p(mask), _p(P), _p(AP), _p(X), _p(R),
                                       _p(partials), _p(rr), _s(X)), "lmg_block_cg_step")


def block_cg_direction(rz_new, rz_old, mask, Z, P):
    """P = Z + beta P with beta_j = rz_new[j] / rz_old[j] for the columns with mask[j] != 0, the bits of axpby(1, z, beta, p);
    the other columns of P are not stored.  rz_new and rz_old are two arrays: the caller alternates between them."""
    k = _block_same_shape("block_cg_direction", Z, P)
    _block_scalars_ok(k, rz_new, rz_old, mask)
    check(_lib.lib().lmg_block_cg_direction(k, P.shape[0], _p(rz_new), _p(rz_old), _p(mask), _p(Z), _p(P), _s(P)),
          "lmg_block_cg_direction")


def block_multi_partials_count(n, k, nb):
    return int(_lib.lib().lmg_block_multi_partials_count(int(n), int(k), int(nb)))


def _block_basis_ok(name, V, nb, W):
    """A block basis V (nb_max, n, k), contiguous, of which nb blocks are in use, and a block W (n, k); returns (k, ldb)."""
    k = _block_ok(W)
    _vec_ok(V)
    if V.dim() != 3 or tuple(V.shape[1:]) != tuple(W.shape) or not 0 <= int(nb) <= V.shape[0]:
        raise ValueError("%s: a basis %s does not hold %d blocks of shape %s" % (name, tuple(V.shape), nb, tuple(W.shape)))
    if V.data_ptr() % 16:
        raise ValueError("a block must start at a 16-byte aligned address")
    return k, V.shape[1] * V.shape[2]


def block_multi_dot(V, nb, W, partials, out):
    """out[i * k + j] = V[i, :, j] . W[:, j] for i < nb and the k columns in one pass; the bits of multi_dot on contiguous
    copies of column j."""
    k, ldb = _block_basis_ok("block_multi_dot", V, nb, W)
    _vec_ok(partials, out)
    if out.numel() < int(nb) * k or partials.numel() < block_multi_partials_count(W.shape[0], k, nb):
        raise ValueError("block_multi_dot: out or partials too short for %d blocks of %d columns" % (nb, k))
    check(_lib.lib().lmg_block_multi_dot(k, W.shape[0], int(nb), _p(V), ldb, _p(W), _p(partials), _p(out), _s(W)),
          "lmg_block_multi_dot")


def block_multi_axpy(V, counts, coef, W, partials=None, norm2=None, subtract=True):
    """Column j: W[:, j] -= sum_i coef[i * k + j] V[i, :, j], i < counts[j] ascending (subtract=False: +=), the bits of
    multi_axpy with counts[j] rows; a column with counts[j] == 0 is not stored.  counts: k Python ints; coef a DEVICE tensor
    in block_multi_dot's layout.  norm2[j] = |W[:, j]|^2 afterwards for every column, if given (partials needed)."""
    counts = [int(c) for c in counts]
    k, ldb = _block_basis_ok("block_multi_axpy", V, 0, W)
    _vec_ok(coef, partials, norm2)
    if len(counts) != k or min(counts) < 0 or max(counts) > V.shape[0]:
        raise ValueError("block_multi_axpy: counts %s for a block of %d columns and a basis of %d blocks" % (counts, k, V.shape[0]))
    if coef.numel() < max(counts) * k or (norm2 is not None and (
            norm2.numel() < k or partials is None or partials.numel() < block_multi_partials_count(W.shape[0], k, 1))):
        raise ValueError("block_multi_axpy: coef, norm2 or partials too short for %s rows of %d columns" % (counts, k))
    check(_lib.lib().lmg_block_multi_axpy(k, W.shape[0], (ctypes.c_int * k)(*counts), 1 if subtract else 0, _p(V), ldb, _p(coef),
                                          _p(W), _p(partials), _p(norm2), _s(W)), "lmg_block_multi_axpy")


def block_scale(scale, W):
    """W[:, j] = scale[j] * W[:, j] with axpby's bits (scale: k Python floats); a scale of 0.0 stores +0.0 whatever the
    column held."""
    k = _block_ok(W)
    scale = [float(s) for s in scale]
    if len(scale) != k:
        raise ValueError("block_scale: %d factors for a block of %d columns" % (len(scale), k))
    check(_lib.lib().lmg_block_scale(k, W.shape[0], (ctypes.c_double * k)(*scale), _p(W), _s(W)), "lmg_block_scale")


def dense_gemv_block(M, X, Y):
    """Y = M X for a dense (n, m) matrix and blocks X (m, k), Y (n, k): M is read once for the k columns."""
    _vec_ok(M)
    k = _block_ok(X, Y)
    if M.dim() != 2 or X.shape[0] != M.shape[1] or Y.shape[0] != M.shape[0]:
        raise ValueError("dense_gemv_block: M %s, X %s, Y %s" % (tuple(M.shape), tuple(X.shape), tuple(Y.shape)))
    check(_lib.lib().lmg_dense_gemv_block(k, M.shape[0], M.shape[1], _p(M), _p(X), _p(Y), _s(M)), "lmg_dense_gemv_block")


# ---- Gauss-Seidel ---------------------------------------------------------------------
class GSSchedule:
    """Ordered independent sets of rows (level schedule or colour classes)."""

    __slots__ = ("kind", "d_rows", "d_ptr", "h_ptr", "nsets", "max_set", "ell", "twin", "backward")

    def __init__(self, kind, order, ptr, device):
        self.kind = kind
        self.h_ptr = np.ascontiguousarray(ptr, dtype=np.int32)
        self.d_rows = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(device)
        self.d_ptr = torch.from_numpy(self.h_ptr).to(device)
        self.nsets = int(self.h_ptr.size - 1)
        self.max_set = int(np.diff(self.h_ptr).max()) if self.nsets else 0
        self.ell = None              # pattern copy in schedule order, built on first use (see _gs_ell)
        self.twin = None             # "multicolor_device": the ColorSell of the forward schedule, shared with reversed()
        self.backward = False        # "multicolor_device": the colours of `twin` run in reverse

    @classmethod
    def from_device(cls, kind, d_rows, h_ptr):
        """A schedule whose row list was built on the device: d_rows (int32, ordered by set) stays where it is, h_ptr
        is the host copy of the set pointers (the only part the host ever sees)."""
        self = cls.__new__(cls)
        self.kind = kind
        self.h_ptr = np.ascontiguousarray(h_ptr, dtype=np.int32)
        self.d_rows = d_rows.contiguous()
        self.d_ptr = torch.from_numpy(self.h_ptr).to(d_rows.device)
        self.nsets = int(self.h_ptr.size - 1)
        self.max_set = int(np.diff(self.h_ptr).max()) if self.nsets else 0
        self.ell, self.twin, self.backward = None, None, False
        return self

    def reversed(self):
        """The same sets in reverse order: on a level schedule (levels of A + A^T) the exact BACKWARD sweep, rows
        n-1 .. 0; on colour classes backward multicolour Gauss-Seidel.  Every executor of csr_gs_schedule follows the
        order of d_rows, so no other kernel is needed.  The copy gets its own schedule-ordered pattern (gs_prepare).
        "multicolor_device": the row list is flipped on the device and the copy shares the ColorSell, whose colours the
        sweep then launches in reverse (the rows of a colour are independent: the same bits as a walk of the flipped list)."""
        ptr = int(self.h_ptr[-1]) - self.h_ptr[::-1] if self.nsets else self.h_ptr
        if self.kind == "multicolor_device":
            out = GSSchedule.from_device(self.kind, torch.flip(self.d_rows, (0,)), ptr)
            out.twin, out.backward = self.twin, not self.backward
            return out
        rows = self.d_rows.cpu().numpy()[::-1]
        return GSSchedule(self.kind, rows, ptr, self.d_rows.device)


def gs_schedule_from_labels(kind, labels, nsets, device):
    order = np.argsort(labels, kind="stable").astype(np.int32)      # ascending row inside a set
    counts = np.bincount(labels, minlength=int(nsets))
    ptr = np.zeros(int(nsets) + 1, dtype=np.int32)
    np.cumsum(counts, out=ptr[1:])
    return GSSchedule(kind, order, ptr, device)


def build_gs_schedule(A_scipy_csr, kind, device, reverse=False):
    """kind = "lexicographic" (level schedule: exact forward sweep) | "multicolor".  reverse=True: the sets in
    reverse order (exact backward sweep / backward multicolour sweep, see GSSchedule.reversed)."""
    A = A_scipy_csr
    n = A.shape[0]
    rp = np.ascontiguousarray(A.indptr, dtype=np.int32)
    ci = np.ascontiguousarray(A.indices, dtype=np.int32)
    lab = np.empty(n, dtype=np.int32)
    L = _lib.lib()
    fn = {"lexicographic": L.lmg_host_gs_levels, "multicolor": L.lmg_host_greedy_colors}.get(kind)
    if fn is None:
        raise ValueError("unknown Gauss-Seidel ordering %r" % (kind,))
    nsets = check(fn(n, rp.ctypes.data, ci.ctypes.data, lab.ctypes.data), "gs schedule")
    sched = gs_schedule_from_labels(kind, lab, nsets, device)
    return sched.reversed() if reverse else sched


def csr_gs_rows(A, x, b, rows):
    _vec_ok(x, b)
    check(_lib.lib().lmg_csr_gs_rows(_p(A.rowptr), _p(A.colidx), _p(A.vals), _p(x), _p(b), _p(rows),
                                     rows.numel(), _s(A.rowptr)), "lmg_csr_gs_rows")


GS_ELL_MAX_SET = 2048            # widest set the one-workgroup ELL executor takes (2 rows per lane);
                                 # measured: at 1025^2 (sets of up to 2050 rows) per-set launches are as fast


def _gs_ell(A, sched):
    """Pattern of A in schedule order for lmg_csr_gs_schedule_ell, or None when the schedule
    does not qualify (chain-like: the one-wave kernel is better; wide sets: per-set launches;
    rows longer than 16 entries).  Built from the DEVICE arrays of the matrix it is used with."""
    total = int(sched.h_ptr[-1]) if sched.nsets else 0
    if total <= 4 * sched.nsets or sched.max_set > GS_ELL_MAX_SET or not A.vals.is_cuda or A.nnz == 0:
        return None
    key = (A.rowptr.data_ptr(), A.colidx.data_ptr(), A.nnz)
    if sched.ell is not None and sched.ell[0] == key:
        return sched.ell
    rows = sched.d_rows.long()
    start = A.rowptr[rows]
    ln = A.rowptr[rows + 1] - start
    kmax = int(ln.max())
    K = next((k for k in (3, 5, 7, 9, 16) if k >= kmax), None)
    if K is None:
        sched.ell = (key, None)
        return sched.ell
    cols = torch.empty((K, total), dtype=I32, device=A.vals.device)
    for j in range(K):
        idx = (start + j).long().clamp(max=A.nnz - 1)
        cols[j] = torch.where(ln > j, A.colidx[idx], sched.d_rows)
    sched.ell = (key, K, sched.d_rows, start.contiguous(), ln.contiguous(), cols.contiguous(), total)
    return sched.ell


_WAVE_GS_ENABLED = True


def set_wavefront_gs_enabled(flag):
    """Whether exact forward Gauss-Seidel on grid-stencil matrices runs the pipelined wavefront kernel
    (default) or the level-scheduled executors (A/B runs and parity tests)."""
    global _WAVE_GS_ENABLED
    _WAVE_GS_ENABLED = bool(flag)


GS_DIRECTIONS = ("forward", "backward")


def _gs_direction(direction):
    if direction not in GS_DIRECTIONS:
        raise ValueError("unknown Gauss-Seidel sweep direction %r (expected 'forward' or 'backward')" % (direction,))
    return direction


def stencil_gs_available(A, direction="forward"):
    """Whether stencil_gs runs on A in this direction.  backward also needs whole lines (n % W == 0): the kernels run
    in mirrored coordinates, which are a plain reversal of the vector only then (ragged grids: reversed schedules)."""
    S = getattr(A, "stencil", None)
    ok = bool(_PACKED_ENABLED and _STENCIL_ENABLED and _WAVE_GS_ENABLED and S is not None and S.gs_ok
              and S.n < GS_WAVE_MAX_ROWS)
    if _gs_direction(direction) == "backward":
        ok = ok and S.n % S.W == 0
    return ok


def stencil_gs(A, x, b, sweeps=1, direction="forward"):
    """`sweeps` exact forward (lexicographic) Gauss-Seidel sweeps in place on x (lmg_stencil_gs_sweep): the
    bits of csr_gs_schedule on the level schedule, without a schedule.  direction="backward": rows n-1 .. 0
    (lmg_stencil_gs_sweep_backward; pyamg's sweep='backward'), the bits of csr_gs_schedule on the reversed level
    schedule; needs stencil_gs_available(A, "backward").

    The band tickets and progress counters live in ONE work buffer per operator (`StencilTwin._gs_work`), shared by both
    directions: sweeps on the same operator must be ordered on one stream (the hierarchy's launch stream); two streams
    sweeping one operator at the same time would race on the counters."""
    _vec_ok(x, b)
    bwd = _gs_direction(direction) == "backward"
    S = A.stencil
    if S is None or not S.gs_ok:
        raise LmgError("stencil_gs needs a grid-stencil matrix without coupling across line ends")
    if bwd and S.n % S.W != 0:
        raise LmgError("backward stencil_gs needs whole grid lines (n %% W == 0): n = %d, W = %d" % (S.n, S.W))
    if S._gs_work is None:
        nb = int(_lib.lib().lmg_stencil_gs_work_bytes(S.n, S.W))
        S._gs_work = torch.zeros((nb + 7) // 8, dtype=torch.int64, device=x.device)
    if sweeps <= 0:
        return
    name = "lmg_stencil_gs_sweep_backward" if bwd else "lmg_stencil_gs_sweep"
    check(getattr(_lib.lib(), name)(*S.c_args(), _p(x), _p(b), _p(S._gs_work), int(sweeps), _s(S.pid)), name)


def stencil_gs_check(A):
    """Raises if a band of the wavefront kernel ever gave up waiting for its predecessor (one D2H read)."""
    S = A.stencil
    if S is not None and S._gs_work is not None:
        if int(S._gs_work.view(torch.int32)[0]):
            raise LmgError("wavefront Gauss-Seidel: a band timed out waiting for the previous one")


COLOR_MAX = 64                   # LMG_COLOR_MAX: colours 0 .. 63 (one 64-bit mask per lane)


def color_device(A):
    """(colour, ncolours, rounds) of the parallel greedy colouring of the square DeviceCSR A (csrc/color.hip): colour is an
    int32 device tensor, one entry per row.  The graph is the pattern of A and A^T without the diagonal; per round the
    uncoloured nodes whose key (hash, index) beats every uncoloured neighbour take the smallest colour no coloured
    neighbour has.  The host reads one count per round, so this cannot be captured into a graph.  A node that would need
    colour COLOR_MAX raises LmgError (no partial result: use gs_mode="multicolor" for such a matrix)."""
    if A.shape[0] != A.shape[1]:
        raise ValueError("a colouring needs a square matrix, got %s" % (A.shape,))
    n, dev, L = A.shape[0], A.device, _lib.lib()
    color = torch.full((max(n, 1),), -1, dtype=I32, device=dev)
    if n == 0:
        return color[:0], 0, 0
    T = A.transpose()
    flag = torch.empty(n, dtype=I32, device=dev)
    nb = int(L.lmg_color_blocks(n))
    left = torch.zeros(nb, dtype=I32, device=dev)
    status = nmg2d_status(dev)
    graph = (n, _p(A.rowptr), _pe(A.colidx), _p(T.rowptr), _pe(T.colidx))
    before, rounds = n, 0
    while before > 0:
        check(L.lmg_color_select(*graph, _p(color), _p(flag), _s(color)), "lmg_color_select")
        check(L.lmg_color_assign(*graph, _p(flag), _p(color), _p(left), _p(status), _s(color)), "lmg_color_assign")
        rounds += 1
        now = _scan_rows(left, nb)[1]
        if now >= before:
            word = int(status.item())
            if word != -1:
                raise LmgError("the colouring needs more than %d colours at node %d (use gs_mode='multicolor')"
                               % (COLOR_MAX, word))
            raise RuntimeError("colouring round %d coloured nothing (%d nodes uncoloured)" % (rounds, now))
        before = now
    return color[:n], int(color.max()) + 1, rounds


def build_gs_schedule_device(A):
    """The GSSchedule of kind "multicolor_device" of the DeviceCSR A, with its ColorSell: color_device, the rows ordered by
    (colour, row) with a stable sort on the device, and the twin.  Only the ncolours + 1 colour pointers come to the host;
    neither the pattern nor the row list does."""
    color, nc, _rounds = color_device(A)
    dev = A.device
    if nc == 0:
        sched = GSSchedule.from_device("multicolor_device", torch.empty(0, dtype=I32, device=dev), np.zeros(1, dtype=np.int32))
    else:
        sorted_color, order = torch.sort(color, stable=True)              # ascending row inside a colour
        ptr = torch.searchsorted(sorted_color, torch.arange(nc + 1, dtype=I32, device=dev)).to(I32)
        sched = GSSchedule.from_device("multicolor_device", order.to(I32), ptr.cpu().numpy())
    gs_prepare(A, sched)
    return sched


def _color_twin(A, sched):
    if sched.twin is None:
        fwd = torch.flip(sched.d_rows, (0,)) if sched.backward else sched.d_rows
        h_ptr = int(sched.h_ptr[-1]) - sched.h_ptr[::-1] if sched.backward and sched.nsets else sched.h_ptr
        sched.twin = ColorSell.from_schedule(A, fwd, h_ptr)
    elif sched.twin.key != (A.rowptr.data_ptr(), A.colidx.data_ptr(), A.nnz):
        raise LmgError("this multicolor_device schedule was built for another matrix")
    return sched.twin


def gs_refresh(A, sched):
    """After the values of A changed in place (same pattern): what a schedule holds of them follows.  Only the ColorSell of
    a "multicolor_device" schedule holds values; every other executor reads A.vals."""
    if sched.kind == "multicolor_device" and sched.twin is not None:
        sched.twin.update_values(A)


def gs_prepare(A, sched):
    """Everything csr_gs_schedule would otherwise build lazily on its first call (allocations, a
    device -> host size read): call it at setup so that the sweep itself is capture-safe."""
    if sched.kind == "multicolor_device":
        _color_twin(A, sched)
        return
    _gs_ell(A, sched)


def csr_gs_schedule(A, x, b, sched, sweeps=1):
    _vec_ok(x, b)
    if sched.kind == "multicolor_device":
        if x.numel() != A.shape[0] or b.numel() != A.shape[0]:
            raise ValueError("csr_gs_schedule: x and b must have the %d rows of A" % A.shape[0])
        _color_twin(A, sched).sweep(x, b, sweeps, sched.backward)
        return
    ell = _gs_ell(A, sched)
    if ell is not None and ell[1] is not None:
        _key, K, rows, start, ln, cols, total = ell
        check(_lib.lib().lmg_csr_gs_schedule_ell(x.numel(), _p(A.vals), _p(x), _p(b), _p(rows), _p(start), _p(ln), _p(cols),
                                                 K, total, _p(sched.d_ptr), sched.nsets, int(sweeps), _s(A.vals)),
              "lmg_csr_gs_schedule_ell")
        return
    check(_lib.lib().lmg_csr_gs_schedule(_p(A.rowptr), _p(A.colidx), _p(A.vals), _p(x), _p(b),
                                         _p(sched.d_rows), _p(sched.d_ptr), sched.h_ptr.ctypes.data,
                                         sched.nsets, sched.max_set, int(sweeps), _s(A.rowptr)),
          "lmg_csr_gs_schedule")


# ---- vectors ------------------------------------------------------------------------------
def axpby(alpha, x, beta, y):
    _vec_ok(x, y)
    check(_lib.lib().lmg_axpby(y.numel(), float(alpha), _p(x), float(beta), _p(y), _s(x)), "lmg_axpby")


def vmul(alpha, x, y, out):
    _vec_ok(x, y, out)
    check(_lib.lib().lmg_vmul(out.numel(), float(alpha), _p(x), _p(y), _p(out), _s(x)), "lmg_vmul")


def csr_inverse_diagonal(A):
    """1/a_ii per row (0 where the diagonal is missing or zero); setup-time helper for the
    zero-initial-guess Jacobi sweep.  Duplicate diagonal entries are summed in storage order,
    like in the sweep."""
    n = A.shape[0]
    d = torch.empty(n, dtype=F64, device=A.vals.device)
    check(_lib.lib().lmg_csr_inverse_diagonal(n, _p(A.rowptr), _p(A.colidx), _p(A.vals), _p(d), _s(A.rowptr)),
          "lmg_csr_inverse_diagonal")
    return d


def copy(src, dst):
    _vec_ok(src, dst)
    check(_lib.lib().lmg_copy(dst.numel(), _p(src), _p(dst), _s(src)), "lmg_copy")


def zero(x):
    _vec_ok(x)
    check(_lib.lib().lmg_zero(x.numel(), _p(x), _s(x)), "lmg_zero")


def dot(x, y, partials, out):
    _vec_ok(x, y, partials, out)
    check(_lib.lib().lmg_dot(x.numel(), _p(x), _p(y), _p(partials), _p(out), _s(x)), "lmg_dot")


def krylov_max_vectors():
    """Most basis rows one multi_dot / multi_axpy call takes."""
    return int(_lib.lib().lmg_krylov_max_vectors())


def multi_partials_count(n, k):
    return int(_lib.lib().lmg_multi_partials_count(int(n), int(k)))


def _basis_ok(V, k, w):
    _vec_ok(V, w)
    if V.dim() != 2 or not 0 <= int(k) <= V.shape[0] or w.dim() != 1 or w.numel() > V.shape[1]:
        raise ValueError("basis %s does not hold %d rows of %d elements" % (tuple(V.shape), k, w.numel()))


def multi_dot(V, k, w, partials, out):
    """out[j] = V[j, :n] . w for j < k in one pass over w (n = w.numel(); V is 2-D contiguous, its row stride is ldv)."""
    _basis_ok(V, k, w)
    _vec_ok(partials, out)
    if out.numel() < int(k) or partials.numel() < multi_partials_count(w.numel(), k):
        raise ValueError("multi_dot: out or partials too short for %d columns" % k)
    check(_lib.lib().lmg_multi_dot(w.numel(), int(k), _p(V), V.shape[1], _p(w), _p(partials), _p(out), _s(w)), "lmg_multi_dot")


def multi_axpy(V, k, coef, w, partials=None, norm2=None, subtract=True):
    """w -= sum_j coef[j] V[j, :n] (subtract=False: +=), j ascending, coef a DEVICE tensor; norm2[0] = |w_new|^2 if given."""
    _basis_ok(V, k, w)
    _vec_ok(coef, partials, norm2)
    if coef.numel() < int(k) or (norm2 is not None and (partials is None or partials.numel() < multi_partials_count(w.numel(), k))):
        raise ValueError("multi_axpy: coef or partials too short for %d columns" % k)
    check(_lib.lib().lmg_multi_axpy(w.numel(), int(k), 1 if subtract else 0, _p(V), V.shape[1], _p(coef), _p(w), _p(partials),
                                    _p(norm2), _s(w)), "lmg_multi_axpy")


# ---- the inner Krylov steps of a K-cycle visit (csrc/krylov.hip) --------------------------------------------------------------
K_INNER = ("gcr", "fcg")
# where kcycle_step1 / kcycle_step2 leave their scalars (include/lmg.h: LMG_KC_*)
KCYCLE_SCALARS = ("alpha1", "rho1", "t1", "gamma", "beta", "alpha2", "rho2", "t2", "a")
KCYCLE_FORMS = {"auto": 0, "one": 1, "two": 2}


def kcycle_partials_count(n):
    return int(_lib.lib().lmg_kcycle_partials_count(int(n)))


def kcycle_grid(n):
    """Workgroups of the two-launch form on n rows = shares every product is cut into."""
    return int(_lib.lib().lmg_kcycle_grid(int(n)))


def kcycle_one_launch_max():
    """Largest n whose steps run as one launch under form "auto"."""
    return int(_lib.lib().lmg_kcycle_one_launch_max())


def _kcycle_args(name, k_inner, form, vecs, scal, partials):
    if k_inner not in K_INNER:
        raise ValueError("k_inner must be 'gcr' or 'fcg', got %r" % (k_inner,))
    if form not in KCYCLE_FORMS:
        raise ValueError("%s: form must be 'auto', 'one' or 'two', got %r" % (name, form))
    _vec_ok(*vecs, scal, partials)
    n = vecs[0].numel()
    if any(v.numel() != n for v in vecs) or scal.numel() < len(KCYCLE_SCALARS):
        raise ValueError("%s: vectors of one length and %d scalars are needed" % (name, len(KCYCLE_SCALARS)))
    return n, 1 if k_inner == "gcr" else 0, KCYCLE_FORMS[form]


def kcycle_step1(k_inner, c1, v1, b, rt, scal, partials, form="auto"):
    """First inner step of a K-cycle visit: alpha1 = <p1, b>, rho1 = <p1, v1> with p1 = v1 ("gcr") or c1 ("fcg"),
    t1 = alpha1 / rho1 (0 where rho1 == 0), rt = b - t1 v1; scal[0:3] = (alpha1, rho1, t1), all on the device
    (lmg_kcycle_step1).  partials: kcycle_partials_count(n) doubles of scratch."""
    n, gcr, f = _kcycle_args("kcycle_step1", k_inner, form, (c1, v1, b, rt), scal, partials)
    check(_lib.lib().lmg_kcycle_step1(n, gcr, f, _p(c1), _p(v1), _p(b), _p(rt), _p(scal), _p(partials), partials.numel(), _s(b)),
          "lmg_kcycle_step1")


def kcycle_step2(k_inner, c1, v1, c2, v2, rt, scal, x_out, partials, form="auto"):
    """Second inner step: gamma = <p2, v1>, beta = <p2, v2>, alpha2 = <p2, rt> with p2 = v2 ("gcr") or c2 ("fcg"), the
    coefficients from them and from rho1, t1 in scal, x_out = a c1 + t2 c2; scal[3:9] = (gamma, beta, alpha2, rho2, t2, a)
    (lmg_kcycle_step2).  x_out may be c2."""
    n, gcr, f = _kcycle_args("kcycle_step2", k_inner, form, (c1, v1, c2, v2, rt, x_out), scal, partials)
    check(_lib.lib().lmg_kcycle_step2(n, gcr, f, _p(c1), _p(v1), _p(c2), _p(v2), _p(rt), _p(scal), _p(x_out), _p(partials),
                                      partials.numel(), _s(rt)), "lmg_kcycle_step2")


def gather(idx, x, buf):
    check(_lib.lib().lmg_gather(idx.numel(), _p(idx), _p(x), _p(buf), _s(idx)), "lmg_gather")


def scatter(idx, buf, x):
    check(_lib.lib().lmg_scatter(idx.numel(), _p(idx), _p(buf), _p(x), _s(idx)), "lmg_scatter")


def dense_gemv(M, x, y):
    _vec_ok(M, x, y)
    check(_lib.lib().lmg_dense_gemv(M.shape[0], M.shape[1], _p(M), _p(x), _p(y), _s(M)), "lmg_dense_gemv")


def dense_gemv_blockdiag(M, x, y):
    """M: (nblocks, bs, bs) contiguous; x, y: nblocks*bs."""
    _vec_ok(M, x, y)
    check(_lib.lib().lmg_dense_gemv_blockdiag(M.shape[0], M.shape[1], _p(M), _p(x), _p(y), _s(M)),
          "lmg_dense_gemv_blockdiag")


def dense_gemv_windows(M, x, x_stride, y, y_stride, z=None, z_stride=0, alpha=1.0):
    """y[k*ys + r] = (z[k*zs + r] if z else 0) + alpha * M[k, r, :] . x[k*xs : k*xs + cols]  for the
    (nblocks, rows, cols) stack M; x, y, z are (views into) flat float64 vectors."""
    _vec_ok(M, x, y, z)
    nb, rows, cols = M.shape
    need_x = (nb - 1) * x_stride + cols
    if x.numel() < need_x or y.numel() < (nb - 1) * y_stride + rows or (z is not None and z.numel() < (nb - 1) * z_stride + rows):
        raise ValueError("dense_gemv_windows: a window leaves its vector")
    check(_lib.lib().lmg_dense_gemv_windows(nb, rows, cols, _p(M), _p(x), int(x_stride), _p(z), int(z_stride), float(alpha),
                                            _p(y), int(y_stride), _s(M)), "lmg_dense_gemv_windows")


def dense_gemv_windows_off(M, x, x_offsets, y, y_stride, z=None, z_stride=0, alpha=1.0):
    """dense_gemv_windows with a table of window starts (int32 tensor, one per block) instead of a stride."""
    _vec_ok(M, x, y, z)
    nb, rows, cols = M.shape
    check(_lib.lib().lmg_dense_gemv_windows_off(nb, rows, cols, _p(M), _p(x), _p(x_offsets), _p(z), int(z_stride), float(alpha),
                                                _p(y), int(y_stride), _s(M)), "lmg_dense_gemv_windows_off")


def coarse_front(M, b, perm, y, tail_out):
    """y = blockdiag(M) b[perm[:nI]], tail_out = b[perm[nI:]] in one launch (M: (k, s, s), nI = k * s)."""
    _vec_ok(M, b, y, tail_out)
    check(_lib.lib().lmg_coarse_front(M.shape[0], M.shape[1], _p(M), _p(b), _p(perm), _p(y), tail_out.numel(), _p(tail_out), _s(M)),
          "lmg_coarse_front")


def coarse_back(W, x_tail, x_offsets, z, alpha, perm, out, accumulate, ntail):
    """out[perm[:nI]] (+)= z + alpha * W_k . x_tail[x_offsets[k]:...], out[perm[nI:nI + ntail]] (+)= x_tail[:ntail]."""
    _vec_ok(W, x_tail, z, out)
    nb, rows, cols = W.shape
    check(_lib.lib().lmg_coarse_back(nb, rows, cols, _p(W), _p(x_tail), _p(x_offsets), _p(z), rows, float(alpha), _p(perm),
                                     _p(out), 1 if accumulate else 0, int(ntail), _s(W)), "lmg_coarse_back")


def coarse_front_gather(M, b, idx, y, tail_idx, tail_out):
    """y[k*s + r] = sum_c M_k[r][c] b[idx[k*s + c]] (idx < 0: 0), tail_out = b[tail_idx] in one launch (M: (k, s, s))."""
    _vec_ok(M, b, y, tail_out)
    check(_lib.lib().lmg_coarse_front_gather(M.shape[0], M.shape[1], _p(M), _p(b), _p(idx), _p(y), tail_idx.numel(),
                                             _p(tail_idx), _p(tail_out), _s(M)), "lmg_coarse_front_gather")


def coarse_back_gather(W, x_tail, xidx, z, alpha, oidx, tail_idx, out, accumulate):
    """out[oidx[k*s + r]] (+)= z[k*s + r] + alpha * sum_c W_k[r][c] x_tail[xidx[k*cw + c]]  (oidx < 0: skipped),
    out[tail_idx[i]] (+)= x_tail[i] (W: (k, s, cw))."""
    _vec_ok(W, x_tail, z, out)
    nb, rows, cols = W.shape
    check(_lib.lib().lmg_coarse_back_gather(nb, rows, cols, _p(W), _p(x_tail), _p(xidx), _p(z), rows, float(alpha), _p(oidx),
                                            _p(out), 1 if accumulate else 0, tail_idx.numel(), _p(tail_idx), _s(W)),
          "lmg_coarse_back_gather")


def _mat_view(t):
    """(batch, rows, cols, ld, batch stride, data pointer) of a 2-D / 3-D float64 device tensor whose rows are contiguous
    (any leading dimension, any batch stride: sub-blocks of larger matrices)."""
    if t.dtype != F64 or not t.is_cuda or t.dim() not in (2, 3) or t.stride(-1) != 1 and t.shape[-1] > 1:
        raise TypeError("expected a float64 device matrix with contiguous rows")
    if t.dim() == 2:
        return 1, t.shape[0], t.shape[1], max(t.stride(0), t.shape[1]), 0, t.data_ptr()
    return t.shape[0], t.shape[1], t.shape[2], max(t.stride(1), t.shape[2]), t.stride(0), t.data_ptr()


def gemm(A, B, C, alpha=1.0, beta=0.0):
    """C = alpha * A @ B + beta * C on (batches of) strided matrix views (lmg_batched_gemm): the coarse-solver setup's
    products without a BLAS library (whose first use costs more than the setup itself in a fresh process)."""
    ba, M, K, lda, sa, pa = _mat_view(A)
    bb, K2, N, ldb, sb, pb = _mat_view(B)
    bc, M2, N2, ldc, sc, pc = _mat_view(C)
    if K != K2 or M != M2 or N != N2 or len({ba, bb, bc} - {1}) > 1:
        raise ValueError("gemm: shapes %s @ %s -> %s" % (tuple(A.shape), tuple(B.shape), tuple(C.shape)))
    batch = max(ba, bb, bc)
    if bc != batch:
        raise ValueError("gemm: the result needs the batch dimension")
    check(_lib.lib().lmg_batched_gemm(batch, M, N, K, float(alpha), pa, lda, sa if ba > 1 else 0, pb, ldb, sb if bb > 1 else 0,
                                      float(beta), pc, ldc, sc, _s(C)), "lmg_batched_gemm")
    return C


def copy2d(src, dst, alpha=1.0, accumulate=False):
    """dst (+)= alpha * src on (batches of) strided matrix views of equal shape (lmg_copy2d)."""
    bs, R, Cc, lds, ss, ps = _mat_view(src)
    bd, R2, C2, ldd, sd, pd = _mat_view(dst)
    if (bs, R, Cc) != (bd, R2, C2):
        raise ValueError("copy2d: shapes %s -> %s" % (tuple(src.shape), tuple(dst.shape)))
    check(_lib.lib().lmg_copy2d(bs, R, Cc, float(alpha), ps, lds, ss, pd, ldd, sd, 1 if accumulate else 0, _s(dst)), "lmg_copy2d")
    return dst


def csr_to_dense(A, dense):
    check(_lib.lib().lmg_csr_to_dense(A.shape[0], A.shape[1], _p(A.rowptr), _p(A.colidx), _p(A.vals), _p(dense), _s(A.rowptr)),
          "lmg_csr_to_dense")


BATCHED_INVERSE_MAX = 128


def batched_inverse(A):
    """Inverses of a stack (nmat, n, n) of small dense matrices, n <= 128 (lmg_batched_inverse: Gauss-Jordan
    with partial pivoting, one workgroup per matrix); None when a pivot is exactly zero."""
    A = A.contiguous()
    nmat, n, _ = A.shape
    out = torch.empty_like(A)
    info = torch.zeros(max(nmat, 1), dtype=I32, device=A.device)
    check(_lib.lib().lmg_batched_inverse(nmat, n, _p(A), _p(out), _p(info), _s(A)), "lmg_batched_inverse")
    return None if info.cpu().numpy().any() else out            # (a library reduction kernel costs 0.1 s to load)


def block_copy(nblocks, bs, src, src_stride, dst, dst_stride):
    _vec_ok(src, dst)
    if src.numel() < (nblocks - 1) * src_stride + bs or dst.numel() < (nblocks - 1) * dst_stride + bs:
        raise ValueError("block_copy: a block leaves its vector")
    check(_lib.lib().lmg_block_copy(int(nblocks), int(bs), _p(src), int(src_stride), _p(dst), int(dst_stride), _s(src)),
          "lmg_block_copy")


# ---- SpGEMM ---------------------------------------------------------------------------------
def exclusive_scan_i32(inp, out):
    n = inp.numel()
    sc = torch.empty(int(_lib.lib().lmg_scan_scratch_count(n)), dtype=I32, device=inp.device)
    check(_lib.lib().lmg_exclusive_scan_i32(n, _p(inp), _p(out), _p(sc), _s(inp)), "lmg_exclusive_scan_i32")


SPGEMM_MAX_ROW_PRODUCTS = 8192       # LMG_SPGEMM_MAX_ROW_PRODUCTS
_LONG_ROW_SETS = 32


SPGEMM_RECORD_MAX_BYTES = 64 << 30   # upper limit of one plan's recorded product map


class SpGEMMPlan:
    """Symbolic result of C = A*B (pattern of C + per-row product counts); `numeric`
    can be re-run when only the values of A or B changed (Galerkin rebuild).  Rows that
    need more products than the LDS kernels hold go through lmg_spgemm_long_rows.

    record: "lazy" (default) -- the first RE-run of `numeric` also records where every product
    lands (2 B per product, lmg_spgemm_numeric_record) and all later runs replay that map
    without sorting; True -- record on the first run already; False -- always sort.  The map is
    only kept when it fits SPGEMM_RECORD_MAX_BYTES and half of the free device memory."""

    def __init__(self, A, B, record="lazy"):
        self.record = record
        self._runs = 0
        self._rec = None             # (prod_ptr, dst, segend, c_colidx)
        self._init_symbolic(A, B)

    def _init_symbolic(self, A, B):
        if A.shape[1] != B.shape[0]:
            raise ValueError("spgemm shape mismatch %s x %s" % (A.shape, B.shape))
        dev = A.device
        n = A.shape[0]
        L = _lib.lib()
        self.shape = (A.shape[0], B.shape[1])
        self.row_products = torch.empty(max(n, 1), dtype=I32, device=dev)
        mx = torch.zeros(1, dtype=I32, device=dev)
        check(L.lmg_spgemm_count(n, _p(A.rowptr), _p(A.colidx), _p(B.rowptr), _p(self.row_products),
                                 _p(mx), _s(A.rowptr)), "lmg_spgemm_count")
        self.max_products = int(mx.item())
        rownnz = torch.zeros(max(n, 1), dtype=I32, device=dev)
        check(L.lmg_spgemm_symbolic(n, _p(A.rowptr), _p(A.colidx), _p(B.rowptr), _p(B.colidx),
                                    _p(self.row_products), self.max_products, _p(rownnz), _s(A.rowptr)),
              "lmg_spgemm_symbolic")
        self.long_rows = None
        if self.max_products > SPGEMM_MAX_ROW_PRODUCTS:
            self.long_rows = torch.nonzero(self.row_products[:n] > SPGEMM_MAX_ROW_PRODUCTS).flatten().to(I32)
            self._long(False, A, B, rownnz, None)
        self.c_rowptr = torch.empty(n + 1, dtype=I32, device=dev)
        exclusive_scan_i32(rownnz[:n], self.c_rowptr)
        self.c_nnz = int(self.c_rowptr[-1].item())

    def _long(self, numeric, A, B, rownnz, out):
        nsets = min(_LONG_ROW_SETS, int(self.long_rows.numel()))
        bc = B.shape[1]
        mark = torch.zeros(nsets * bc, dtype=I32, device=A.device)
        val = torch.empty(nsets * bc, dtype=F64, device=A.device) if numeric else None
        check(_lib.lib().lmg_spgemm_long_rows(
            1 if numeric else 0, self.long_rows.numel(), _p(self.long_rows), _p(A.rowptr), _p(A.colidx),
            _p(A.vals), _p(B.rowptr), _p(B.colidx), _p(B.vals), bc, nsets, _p(val), _p(mark), _p(rownnz),
            _p(out.rowptr) if out is not None else None, _p(out.colidx) if out is not None else None,
            _p(out.vals) if out is not None else None, _s(self.long_rows)), "lmg_spgemm_long_rows")

    def _record_buffers(self, dev):
        """Buffers of the product map, or None when recording is off / does not fit."""
        n = self.shape[0]
        short = torch.where(self.row_products[:n] <= SPGEMM_MAX_ROW_PRODUCTS, self.row_products[:n],
                            torch.zeros_like(self.row_products[:n])).long()
        incl = torch.cumsum(short, 0)
        total = int(incl[-1]) if n else 0
        need = 2 * total + 2 * self.c_nnz + 8 * n
        limit = SPGEMM_RECORD_MAX_BYTES
        if dev.type == "cuda":
            limit = min(limit, torch.cuda.mem_get_info(dev)[0] // 2)
        if total == 0 or need > limit:
            return None
        prod_ptr = (incl - short).contiguous()
        return (prod_ptr, torch.empty(total, dtype=torch.int16, device=dev),
                torch.zeros(max(self.c_nnz, 1), dtype=torch.int16, device=dev))

    def numeric(self, A, B, out=None):
        dev = A.device
        L = _lib.lib()
        self._runs += 1
        if self._rec is not None:
            prod_ptr, dst, segend, c_colidx = self._rec
            if out is None:
                out = DeviceCSR(self.c_rowptr, c_colidx, torch.empty(self.c_nnz, dtype=F64, device=dev), self.shape)
            elif out.colidx is not c_colidx:
                out.colidx.copy_(c_colidx)
            check(L.lmg_spgemm_numeric_replay(A.shape[0], _p(A.rowptr), _p(A.colidx), _p(A.vals), _p(B.rowptr),
                                              _p(B.vals), _p(self.row_products), self.max_products, _p(out.rowptr),
                                              _p(out.vals), _p(prod_ptr), _p(dst), _p(segend), _s(A.rowptr)),
                  "lmg_spgemm_numeric_replay")
            if self.long_rows is not None:
                self._long(True, A, B, None, out)
            return out
        if out is None:
            out = DeviceCSR(self.c_rowptr, torch.empty(self.c_nnz, dtype=I32, device=dev),
                            torch.empty(self.c_nnz, dtype=F64, device=dev), self.shape)
        bufs = None
        if self.record is True or (self.record == "lazy" and self._runs >= 2):
            bufs = self._record_buffers(dev)
            if bufs is None:
                self.record = False                      # does not fit: stop asking
        if bufs is not None:
            prod_ptr, dst, segend = bufs
            check(L.lmg_spgemm_numeric_record(A.shape[0], _p(A.rowptr), _p(A.colidx), _p(A.vals), _p(B.rowptr),
                                              _p(B.colidx), _p(B.vals), _p(self.row_products), self.max_products,
                                              _p(out.rowptr), _p(out.colidx), _p(out.vals), _p(prod_ptr), _p(dst),
                                              _p(segend), _s(A.rowptr)), "lmg_spgemm_numeric_record")
            self._rec = (prod_ptr, dst, segend, out.colidx)
        else:
            check(L.lmg_spgemm_numeric(A.shape[0], _p(A.rowptr), _p(A.colidx), _p(A.vals),
                                       _p(B.rowptr), _p(B.colidx), _p(B.vals),
                                       _p(self.row_products), self.max_products,
                                       _p(out.rowptr), _p(out.colidx), _p(out.vals), _s(A.rowptr)),
                  "lmg_spgemm_numeric")
        if self.long_rows is not None:
            self._long(True, A, B, None, out)
        return out

    def recorded_bytes(self):
        return 0 if self._rec is None else sum(int(t.numel()) * t.element_size() for t in self._rec[:3])


def spgemm(A, B):
    return SpGEMMPlan(A, B).numeric(A, B)


# ---- 2-D learned transfers (csrc/nmg2d.hip; the stages: learned_q2d.py) -----------------------
NMG2D_RULES = {1: "negative_offdiagonal", 2: "diagonal", 3: "valence", 4: "few_neighbours", 5: "isolated_neighbour",
               6: "second_neighbours", 7: "index_range"}        # lmg_nmg2d_rule


def host_greedy_cf(A):
    """is_coarse (int32, n) of the SciPy CSR matrix A by lmg_host_greedy_cf: node i is coarse iff no coarse c < i has
    A[c, i] > 0."""
    rp, ci = np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32)
    va = np.ascontiguousarray(A.data, dtype=np.float64)
    out = np.empty(A.shape[0], dtype=np.int32)
    check(_lib.lib().lmg_host_greedy_cf(A.shape[0], rp.ctypes.data, ci.ctypes.data, va.ctypes.data, out.ctypes.data),
          "lmg_host_greedy_cf")
    return out


def nmg2d_status(device):
    """The status word of one stage, set to "nothing refused" (all bits)."""
    return torch.full((1,), -1, dtype=torch.int64, device=device)


def nmg2d_read_status(status):
    """None, or (rule name, order) of the first refusal: one read back (it synchronises)."""
    word = int(status.item())
    return None if word == -1 else (NMG2D_RULES.get(word & 0xFF, "rule %d" % (word & 0xFF)), word >> 8)


def _i32_ok(*ts):
    for t in ts:
        if t.dtype != I32 or not t.is_contiguous() or not t.is_cuda:
            raise TypeError("expected contiguous int32 device tensors, got %s %s" % (t.dtype, t.device))


def nmg2d_check(A, status):
    check(_lib.lib().lmg_nmg2d_check(A.shape[0], _p(A.rowptr), _p(A.colidx), _p(A.vals), _p(status), _s(A.vals)),
          "lmg_nmg2d_check")


def nmg2d_count(A, coarse_nodes, extra, status):
    _i32_ok(coarse_nodes, extra)
    if extra.numel() != coarse_nodes.numel():
        raise ValueError("extra must have one entry per coarse node")
    check(_lib.lib().lmg_nmg2d_count(coarse_nodes.numel(), _p(coarse_nodes), _p(A.rowptr), _p(A.colidx), _p(A.vals),
                                     _p(extra), _p(status), _s(A.vals)), "lmg_nmg2d_count")


def nmg2d_patches(A, patch_node, patch_variant, rank, patches, fill_idx, status):
    _i32_ok(patch_node, patch_variant, rank, fill_idx)
    _vec_ok(patches)
    p = patch_node.numel()
    if patch_variant.numel() != p or rank.numel() != A.shape[0] or patches.numel() != 43 * p or fill_idx.numel() != 31 * p:
        raise ValueError("nmg2d_patches: inconsistent array sizes")
    check(_lib.lib().lmg_nmg2d_patches(p, _p(patch_node), _p(patch_variant), A.shape[0], _p(A.rowptr), _p(A.colidx),
                                       _p(A.vals), _p(rank), _p(patches), _p(fill_idx), _p(status), _s(A.vals)),
          "lmg_nmg2d_patches")


def nmg2d_contrib(nc, fill_idx, rank, keys, status):
    _i32_ok(fill_idx, rank)
    p = fill_idx.numel() // 31
    if fill_idx.numel() != 31 * p or keys.dtype != torch.int64 or keys.numel() != 31 * p or not keys.is_contiguous():
        raise ValueError("nmg2d_contrib: inconsistent array sizes")
    check(_lib.lib().lmg_nmg2d_contrib(p, rank.numel(), nc, _p(fill_idx), _p(rank), _p(keys), _p(status), _s(fill_idx)),
          "lmg_nmg2d_contrib")


def nmg2d_fold(start, keys, slot, res, nc, row, col, val):
    _i32_ok(row, col)
    _vec_ok(res, val)
    ne = start.numel() - 1
    if (start.dtype, keys.dtype, slot.dtype) != (torch.int64,) * 3 or min(row.numel(), col.numel(), val.numel()) < ne \
            or keys.numel() != slot.numel() or res.numel() != keys.numel():
        raise ValueError("nmg2d_fold: inconsistent arrays")
    check(_lib.lib().lmg_nmg2d_fold(ne, _p(start.contiguous()), _p(keys.contiguous()), _p(slot.contiguous()), _p(res), nc,
                                    _p(row), _p(col), _p(val), _s(res)), "lmg_nmg2d_fold")


def nmg2d_normalize(B):
    """Q: the DeviceCSR B with every row divided by its sum (pattern arrays shared with B)."""
    q = torch.empty_like(B.vals)
    check(_lib.lib().lmg_nmg2d_normalize(B.shape[0], _p(B.rowptr), _p(B.vals), _p(q), _s(B.vals)), "lmg_nmg2d_normalize")
    return DeviceCSR(B.rowptr, B.colidx, q, B.shape)


def nmg2d_dneighs(last_patch, fill_idx, rank, d_neighs):
    _i32_ok(last_patch, fill_idx, rank, d_neighs)
    nc = last_patch.numel()
    if d_neighs.numel() != 6 * nc or fill_idx.numel() % 31:
        raise ValueError("nmg2d_dneighs: inconsistent array sizes")
    check(_lib.lib().lmg_nmg2d_dneighs(nc, _p(last_patch), _p(fill_idx), _p(rank), _p(d_neighs), _s(rank)), "lmg_nmg2d_dneighs")


def nmg2d_cut(A, d_neighs):
    """The DeviceCSR A without the entries (i, j) with j != i and j not in d_neighs[i] ((n, 6) int32, padded with -1)."""
    _i32_ok(d_neighs)
    n = A.shape[0]
    if d_neighs.numel() != 6 * n:
        raise ValueError("d_neighs must be (n, 6)")
    L, dev = _lib.lib(), A.device
    rownnz = torch.empty(max(n, 1), dtype=I32, device=dev)
    check(L.lmg_nmg2d_cut_mark(n, _p(A.rowptr), _p(A.colidx), _p(d_neighs), _p(rownnz), _s(A.vals)), "lmg_nmg2d_cut_mark")
    rp = torch.empty(n + 1, dtype=I32, device=dev)
    exclusive_scan_i32(rownnz[:n], rp)
    nnz = int(rp[-1].item())
    cj, cv = torch.empty(nnz, dtype=I32, device=dev), torch.empty(nnz, dtype=F64, device=dev)
    check(L.lmg_nmg2d_cut_fill(n, _p(A.rowptr), _p(A.colidx), _p(A.vals), _p(d_neighs), _p(rp), _p(cj), _p(cv), _s(A.vals)),
          "lmg_nmg2d_cut_fill")
    return DeviceCSR(rp, cj, cv, A.shape)


# ---- classical AMG setup (csrc/amg.hip; the stages: amg.py) -------------------------------------
AMG_UNDECIDED, AMG_COARSE, AMG_FINE, AMG_FINE0 = 0, 1, 2, 3          # lmg_amg_state
AMG_RULES = {1: "pivot", 2: "candidate", 3: "members"}                 # lmg_amg_rule


def _pe(t):
    """The address of an entry array for an entry point that refuses null pointers: a matrix without entries hands in a
    one-element array of its own (an empty tensor has no address)."""
    return _p(t if t.numel() else torch.empty(1, dtype=t.dtype, device=t.device))


def _scan_rows(rownnz, n):
    """(rowptr (n + 1), total) of the per-row counts: the scan, and the one read back of its last element."""
    rp = torch.empty(n + 1, dtype=I32, device=rownnz.device)
    exclusive_scan_i32(rownnz[:n], rp)
    return rp, int(rp[-1].item())


def amg_strength(A, theta):
    """(s_rowptr, s_colidx) of the strength pattern S of the DeviceCSR A: count, scan, fill."""
    n, dev, L = A.shape[0], A.device, _lib.lib()
    rownnz = torch.empty(max(n, 1), dtype=I32, device=dev)
    check(L.lmg_amg_strength_count(n, _p(A.rowptr), _pe(A.colidx), _pe(A.vals), float(theta), _p(rownnz), _s(A.vals)),
          "lmg_amg_strength_count")
    rp, nnz = _scan_rows(rownnz, n)
    sj = torch.empty(nnz, dtype=I32, device=dev)
    check(L.lmg_amg_strength_fill(n, _p(A.rowptr), _pe(A.colidx), _pe(A.vals), float(theta), _p(rp), _pe(sj), _s(A.vals)),
          "lmg_amg_strength_fill")
    return rp, sj


def amg_pmis_keys(S, ST, count, state, is_coarse):
    _i32_ok(count, state, is_coarse)
    n = S.shape[0]
    if ST.shape != S.shape or min(count.numel(), state.numel(), is_coarse.numel()) < n:
        raise ValueError("amg_pmis_keys: inconsistent array sizes")
    check(_lib.lib().lmg_amg_pmis_keys(n, _p(S.rowptr), _p(ST.rowptr), _p(count), _p(state), _p(is_coarse), _s(state)),
          "lmg_amg_pmis_keys")


def amg_pmis_round(S, ST, count, state, flag, is_coarse, block_undecided):
    """One round: select, then update.  block_undecided (amg_pmis_blocks(n) int32) receives the undecided nodes left."""
    _i32_ok(count, state, flag, is_coarse, block_undecided)
    n, L = S.shape[0], _lib.lib()
    if min(count.numel(), state.numel(), flag.numel(), is_coarse.numel()) < n \
            or block_undecided.numel() < int(L.lmg_amg_pmis_blocks(n)):
        raise ValueError("amg_pmis_round: inconsistent array sizes")
    check(L.lmg_amg_pmis_select(n, _p(S.rowptr), _pe(S.colidx), _p(ST.rowptr), _pe(ST.colidx), _p(count), _p(state), _p(flag),
                                _s(state)), "lmg_amg_pmis_select")
    check(L.lmg_amg_pmis_update(n, _p(S.rowptr), _pe(S.colidx), _p(flag), _p(state), _p(is_coarse), _p(block_undecided),
                                _s(state)), "lmg_amg_pmis_update")


def amg_pmis_blocks(n):
    return int(_lib.lib().lmg_amg_pmis_blocks(n))


def amg_interp(A, S, state, rank, n_c, status):
    """Direct interpolation: the DeviceCSR P (n x n_c).  A refusal is left in `status` (nmg2d_status / amg_read_status)."""
    _i32_ok(state, rank)
    n, dev, L = A.shape[0], A.device, _lib.lib()
    if S.shape != A.shape or state.numel() < n or rank.numel() < n:
        raise ValueError("amg_interp: inconsistent array sizes")
    rownnz = torch.empty(max(n, 1), dtype=I32, device=dev)
    check(L.lmg_amg_interp_count(n, _p(S.rowptr), _pe(S.colidx), _p(state), _p(rownnz), _s(state)), "lmg_amg_interp_count")
    rp, nnz = _scan_rows(rownnz, n)
    pj, pv = torch.empty(nnz, dtype=I32, device=dev), torch.empty(nnz, dtype=F64, device=dev)
    check(L.lmg_amg_interp_fill(n, _p(A.rowptr), _pe(A.colidx), _pe(A.vals), _p(S.rowptr), _pe(S.colidx), _p(state), _p(rank),
                                _p(rp), _pe(pj), _pe(pv), _p(status), _s(state)), "lmg_amg_interp_fill")
    return DeviceCSR(rp, pj, pv, (n, int(n_c)))


def amg_smooth(A, P, AP, state, rank, omega, trunc):
    """One Jacobi step on P with truncation (AP = A P): the new DeviceCSR P."""
    _i32_ok(state, rank)
    n, dev, L = A.shape[0], A.device, _lib.lib()
    if P.shape[0] != n or AP.shape != P.shape or state.numel() < n or rank.numel() < n:
        raise ValueError("amg_smooth: inconsistent array sizes")
    args = (n, _p(A.rowptr), _pe(A.colidx), _pe(A.vals), _p(P.rowptr), _pe(P.colidx), _pe(P.vals), _p(AP.rowptr),
            _pe(AP.colidx), _pe(AP.vals), _p(state), _p(rank), float(omega), float(trunc))
    rownnz = torch.empty(max(n, 1), dtype=I32, device=dev)
    check(L.lmg_amg_smooth_count(*args, _p(rownnz), _s(state)), "lmg_amg_smooth_count")
    rp, nnz = _scan_rows(rownnz, n)
    qj, qv = torch.empty(nnz, dtype=I32, device=dev), torch.empty(nnz, dtype=F64, device=dev)
    check(L.lmg_amg_smooth_fill(*args, _p(rp), _pe(qj), _pe(qv), _s(state)), "lmg_amg_smooth_fill")
    return DeviceCSR(rp, qj, qv, P.shape)


def amg_read_status(status):
    """None, or (rule name, row) of the first refusal: one read back (it synchronises)."""
    word = int(status.item())
    return None if word == -1 else (AMG_RULES.get(word & 0xFF, "rule %d" % (word & 0xFF)), word >> 8)


# ---- smoothed-aggregation setup (csrc/sa.hip; the stages: aggregation.py) ------------------------
SA_UNDECIDED, SA_ROOT, SA_COVERED, SA_ISOLATED = 0, 1, 2, 3          # lmg_sa_state


def _count_scan_fill(n, dev, count, fill):
    """(rowptr, colidx) of a pattern built in the usual three steps: count(rownnz), the scan, fill(rowptr, colidx)."""
    rownnz = torch.empty(max(n, 1), dtype=I32, device=dev)
    count(rownnz)
    rp, nnz = _scan_rows(rownnz, n)
    cj = torch.empty(nnz, dtype=I32, device=dev)
    fill(rp, cj)
    return rp, cj


def sa_strength(A, theta):
    """(s_rowptr, s_colidx) of the symmetric strength pattern S of the DeviceCSR A: the diagonal, count, scan, fill."""
    n, dev, L = A.shape[0], A.device, _lib.lib()
    diag = torch.empty(max(n, 1), dtype=F64, device=dev)
    a = (n, _p(A.rowptr), _pe(A.colidx), _pe(A.vals))
    check(L.lmg_sa_diagonal(*a, _p(diag), _s(A.vals)), "lmg_sa_diagonal")
    return _count_scan_fill(
        n, dev,
        lambda c: check(L.lmg_sa_strength_count(*a, _p(diag), float(theta), _p(c), _s(A.vals)), "lmg_sa_strength_count"),
        lambda rp, sj: check(L.lmg_sa_strength_fill(*a, _p(diag), float(theta), _p(rp), _pe(sj), _s(A.vals)),
                             "lmg_sa_strength_fill"))


def sa_graph(S, ST):
    """(g_rowptr, g_colidx) of the aggregation graph: the merge of the rows of S and ST = S^T without isolated nodes."""
    n, L = S.shape[0], _lib.lib()
    if ST.shape != S.shape:
        raise ValueError("sa_graph: inconsistent array sizes")
    a = (n, _p(S.rowptr), _pe(S.colidx), _p(ST.rowptr), _pe(ST.colidx))
    return _count_scan_fill(
        n, S.device,
        lambda c: check(L.lmg_sa_graph_count(*a, _p(c), _s(c)), "lmg_sa_graph_count"),
        lambda rp, gj: check(L.lmg_sa_graph_fill(*a, _p(rp), _pe(gj), _s(rp)), "lmg_sa_graph_fill"))


def sa_blocks(n):
    return int(_lib.lib().lmg_sa_blocks(n))


def sa_mis2_init(S, state, is_root):
    _i32_ok(state, is_root)
    n = S.shape[0]
    if min(state.numel(), is_root.numel()) < n:
        raise ValueError("sa_mis2_init: inconsistent array sizes")
    check(_lib.lib().lmg_sa_mis2_init(n, _p(S.rowptr), _p(state), _p(is_root), _s(state)), "lmg_sa_mis2_init")


def sa_mis2_round(G, state, t1, flag, c1, is_root, block_undecided):
    """One round: t1, t2, c1, update.  block_undecided (sa_blocks(n) int32) receives the undecided nodes left."""
    _i32_ok(state, t1, flag, c1, is_root, block_undecided)
    n, L = G.shape[0], _lib.lib()
    if min(state.numel(), t1.numel(), flag.numel(), c1.numel(), is_root.numel()) < n \
            or block_undecided.numel() < int(L.lmg_sa_blocks(n)):
        raise ValueError("sa_mis2_round: inconsistent array sizes")
    g, st = (n, _p(G.rowptr), _pe(G.colidx)), _s(state)
    check(L.lmg_sa_mis2_t1(*g, _p(state), _p(t1), st), "lmg_sa_mis2_t1")
    check(L.lmg_sa_mis2_t2(*g, _p(state), _p(t1), _p(flag), st), "lmg_sa_mis2_t2")
    check(L.lmg_sa_mis2_c1(*g, _p(state), _p(flag), _p(c1), st), "lmg_sa_mis2_c1")
    check(L.lmg_sa_mis2_update(*g, _p(flag), _p(c1), _p(state), _p(is_root), _p(block_undecided), st), "lmg_sa_mis2_update")


def sa_assign(G, state, rank, a1, a2):
    """The two assignment phases: a1 (roots and their neighbours), then a2 (the nodes two edges from a root)."""
    _i32_ok(state, rank, a1, a2)
    n, L = G.shape[0], _lib.lib()
    if min(state.numel(), rank.numel(), a1.numel(), a2.numel()) < n:
        raise ValueError("sa_assign: inconsistent array sizes")
    g, st = (n, _p(G.rowptr), _pe(G.colidx)), _s(state)
    check(L.lmg_sa_assign1(*g, _p(state), _p(rank), _p(a1), st), "lmg_sa_assign1")
    check(L.lmg_sa_assign2(*g, _p(state), _p(a1), _p(a2), st), "lmg_sa_assign2")


def sa_tentative(agg, n_agg, B, status):
    """(T, Bc): the tentative prolongator (n x n_agg DeviceCSR, one entry per aggregated row) of the candidate B and the
    coarse candidate.  A refusal is left in `status` (nmg2d_status / amg_read_status)."""
    _i32_ok(agg)
    _vec_ok(B)
    n, dev, L = B.numel(), B.device, _lib.lib()
    n_agg = int(n_agg)
    if agg.numel() < n or not 0 < n_agg <= n:
        raise ValueError("sa_tentative: inconsistent array sizes")
    st = _s(B)
    vals = []

    def pattern(rp, tj):
        vals.append(torch.empty(tj.numel(), dtype=F64, device=dev))
        check(L.lmg_sa_tentative_pattern(n, n_agg, _p(agg), _p(B), _p(rp), _pe(tj), _pe(vals[0]), st), "lmg_sa_tentative_pattern")

    rp, tj = _count_scan_fill(n, dev, lambda c: check(L.lmg_sa_tentative_count(n, n_agg, _p(agg), _p(c), st),
                                                      "lmg_sa_tentative_count"), pattern)
    members = DeviceCSR(rp, tj, vals[0], (n, n_agg)).transpose()
    Bc = torch.empty(n_agg, dtype=F64, device=dev)
    check(L.lmg_sa_norms(n_agg, _p(members.rowptr), _pe(members.colidx), _pe(members.vals), _p(Bc), _p(status), st),
          "lmg_sa_norms")
    tv = torch.empty_like(vals[0])
    check(L.lmg_sa_tentative_fill(n, n_agg, _p(agg), _p(B), _p(Bc), _p(rp), _pe(tv), st), "lmg_sa_tentative_fill")
    return DeviceCSR(rp, tj, tv, (n, n_agg)), Bc


def sa_row_states(T):
    """int32 per row of T: AMG_FINE where the row has an entry, AMG_FINE0 where it is empty (what amg_smooth reads)."""
    n = T.shape[0]
    state = torch.empty(max(n, 1), dtype=I32, device=T.device)
    check(_lib.lib().lmg_sa_row_states(n, _p(T.rowptr), _p(state), _s(state)), "lmg_sa_row_states")
    return state


# ---- smoothed aggregation for systems (csrc/nsp.hip; the stages: aggregation.py) -------------------
NSP_MAX_CANDIDATES = 6                                                 # LMG_NSP_MAX_CANDIDATES


def nsp_condense(A, bs):
    """C, the condensed DeviceCSR (N x N, N = n / bs) of the node blocks of A: c_IJ the Frobenius norm of block (I, J),
    an entry wherever the block stores one.  Count, scan, fill."""
    n, dev, L, bs = A.shape[0], A.device, _lib.lib(), int(bs)
    if bs < 1 or n % bs or A.shape[1] != n:
        raise ValueError("nsp_condense: a square matrix of n = block_size * nodes rows, got %s and %d" % (A.shape, bs))
    N, st = n // bs, _s(A.vals)
    vals = []

    def fill(rp, cj):
        vals.append(torch.empty(cj.numel(), dtype=F64, device=dev))
        check(L.lmg_nsp_condense_fill(N, bs, _p(A.rowptr), _pe(A.colidx), _pe(A.vals), _p(rp), _pe(cj), _pe(vals[0]), st),
              "lmg_nsp_condense_fill")

    rp, cj = _count_scan_fill(N, dev, lambda c: check(L.lmg_nsp_condense_count(N, bs, _p(A.rowptr), _pe(A.colidx), _p(c), st),
                                                      "lmg_nsp_condense_count"), fill)
    return DeviceCSR(rp, cj, vals[0], (N, N))


def nsp_tentative(agg_nodes, n_agg, bs, X, rank_tol, status):
    """(T, Bc): the tentative prolongator (n x k n_agg DeviceCSR, k entries per row of an aggregated node) of the candidates
    X (n x k, row-major) by two rounds of Cholesky-QR per aggregate, and the coarse candidates (k n_agg x k).  agg_nodes:
    the aggregate per NODE of bs unknowns.  status: TWO words (nmg2d_status semantics), one per round; refusals are left
    there (amg_read_status on status[0:1], then on status[1:2])."""
    _i32_ok(agg_nodes)
    if X.dtype != F64 or X.dim() != 2 or not X.is_contiguous() or not X.is_cuda:
        raise TypeError("expected a contiguous fp64 (n, k) device tensor, got %s %s" % (X.dtype, tuple(X.shape)))
    n, k = X.shape
    dev, L, bs, n_agg = X.device, _lib.lib(), int(bs), int(n_agg)
    if bs < 1 or n % bs or not 1 <= k <= NSP_MAX_CANDIDATES or agg_nodes.numel() < n // bs or not 0 < n_agg <= n // bs \
            or status.numel() != 2:
        raise ValueError("nsp_tentative: inconsistent array sizes")
    N, st, rank_tol = n // bs, _s(X), float(rank_tol)
    # the member nodes of every aggregate, ascending: the transpose of the node pattern (one entry per aggregated node)
    ones = torch.ones(N, dtype=F64, device=dev)
    vals = []

    def pattern(rp, tj):
        vals.append(torch.empty(tj.numel(), dtype=F64, device=dev))
        check(L.lmg_sa_tentative_pattern(N, n_agg, _p(agg_nodes), _p(ones), _p(rp), _pe(tj), _pe(vals[0]), st),
              "lmg_sa_tentative_pattern")

    rp, tj = _count_scan_fill(N, dev, lambda c: check(L.lmg_sa_tentative_count(N, n_agg, _p(agg_nodes), _p(c), st),
                                                      "lmg_sa_tentative_count"), pattern)
    members = DeviceCSR(rp, tj, vals[0], (N, n_agg)).transpose()
    m = (_p(members.rowptr), _pe(members.colidx))
    R1, R2 = (torch.empty(n_agg * k * k, dtype=F64, device=dev) for _ in range(2))
    Y = torch.zeros(n, k, dtype=F64, device=dev)
    check(L.lmg_nsp_gram_chol(n_agg, N, bs, k, *m, _p(X), rank_tol, _p(R1), _p(status[0:1]), st), "lmg_nsp_gram_chol")
    check(L.lmg_nsp_apply(n, n_agg, bs, k, _p(agg_nodes), _p(X), _p(R1), _p(Y), st), "lmg_nsp_apply")
    check(L.lmg_nsp_gram_chol(n_agg, N, bs, k, *m, _p(Y), rank_tol, _p(R2), _p(status[1:2]), st), "lmg_nsp_gram_chol")
    Bc = torch.empty(n_agg * k, k, dtype=F64, device=dev)
    check(L.lmg_nsp_tri_product(n_agg, k, _p(R2), _p(R1), _p(Bc), st), "lmg_nsp_tri_product")
    tv = []

    def fill(rp, tj):
        tv.append(torch.empty(tj.numel(), dtype=F64, device=dev))
        check(L.lmg_nsp_tentative_fill(n, n_agg, bs, k, _p(agg_nodes), _p(Y), _p(R2), _p(rp), _pe(tj), _pe(tv[0]), st),
              "lmg_nsp_tentative_fill")

    rp, tj = _count_scan_fill(n, dev, lambda c: check(L.lmg_nsp_tentative_count(n, n_agg, bs, k, _p(agg_nodes), _p(c), st),
                                                      "lmg_nsp_tentative_count"), fill)
    return DeviceCSR(rp, tj, tv[0], (n, k * n_agg)), Bc


# ---- hipGraph ---------------------------------------------------------------------------------
class CapturedGraph:
    """A launch sequence captured on the current stream (lmg_graph_*), replayable."""

    def __init__(self):
        self._exec = ctypes.c_void_p(None)

    def __enter__(self):
        check(_lib.lib().lmg_graph_begin(_s()), "lmg_graph_begin")
        return self

    def __exit__(self, et, ev, tb):
        rc = _lib.lib().lmg_graph_end(_s(), ctypes.byref(self._exec))
        if et is None:
            check(rc, "lmg_graph_end")
        return False

    def launch(self):
        check(_lib.lib().lmg_graph_launch(self._exec, _s()), "lmg_graph_launch")

    def __del__(self):
        try:
            if self._exec:
                _lib.lib().lmg_graph_destroy(self._exec)
        except Exception:
            pass


# ---- torch.ops.lmg.* registration ------------------------------------------------------------
def register_torch_ops():
    """Expose the kernels as PyTorch custom ops taking ROCm tensors, torch.ops.lmg.* (torch_ops.py)."""
    from . import torch_ops          # (imports this module)
    torch_ops.register()
