"""The lossless storage twins of a DeviceCSR (ops.py) that the sweep kernels and the fused passes read, and the host-side
decoding of a verified pattern table into the grid views of it:

  PackedCSR, SellCSR, RowPatterns     what lmg_pcsr_sweep / lmg_sell_sweep / lmg_rpat_sweep_grid run on
  StencilTwin                         3x3-window view of a RowPatterns twin (lmg_stencil_sweep and the fused passes)
  ProlongTwin, RestrictTwin           2x2- / 3x3-window views of the row patterns of grid transfers (fused passes)
  DiaTwin                             slot arrays of grid operators with per-row values (lmg_dia_smooth)
  ColorSell                           the matrix in the order of a colour schedule, sliced ELL (lmg_color_sweep)

Every class builds itself from device arrays and knows the C arguments that describe it (sweep_args, c_args).  WHICH twin
an operator gets, and which kernel then runs, is decided in ops.py (DeviceCSR.pack, the switches and thresholds there):
nothing here reads a switch.  The decisions that ARE taken here -- window slots, line stride, hot patterns -- are the plain
functions below, over NumPy arrays and Python ints: they run (and are tested) without a device.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import LmgError, check

F64 = torch.float64
F32 = torch.float32
I32 = torch.int32
VALUES = ("f64", "f32")        # how a SELL / DIA twin stores its values (the vectors and the arithmetic are fp64 either way)


def check_values(values, what="values"):
    """`values` if it is one of VALUES, else a ValueError (reads no state: callers check before they build anything)."""
    if values not in VALUES:
        raise ValueError("%s must be one of %s, got %r" % (what, VALUES, values))
    return values


def _s(*ts):
    """The HIP stream the launch goes to: the current stream of the device that holds the tensors (the first
    device tensor among `ts`), or of the current device when none is given."""
    for t in ts:
        if t is not None and getattr(t, "is_cuda", False):
            if t.device.index != torch.cuda.current_device():
                # a HIP launch goes to the CURRENT device: refuse loudly instead of launching there with another
                # device's pointers (the solver classes switch devices themselves: solvers.Solver.on_device)
                raise LmgError("operands live on %s but the current device is cuda:%d: wrap the call in "
                               "torch.cuda.device(...)" % (t.device, torch.cuda.current_device()))
            return torch.cuda.current_stream(t.device).cuda_stream
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


# ---- decoding a pattern table: ptr[npat + 1], off[nent] (column - base(row), int64), val[nent] -----------------------------
def _decompose(off, W, radius=1):
    """(c, d) of a linear offset for line stride W, |c|, |d| <= radius, or None."""
    for c in range(-radius, radius + 1):
        d = off - c * W
        if -radius <= d <= radius:
            return c, d
    return None


def slot_3x3(W):
    """Offset -> slot number 3 (c + 1) + (d + 1) of the 3x3 window  c * W + d, c, d in {-1, 0, 1}  (None: no slot)."""
    def slot(off):
        cd = _decompose(off, W)
        return None if cd is None else (cd[0] + 1) * 3 + (cd[1] + 1)
    return slot


def slot_2x2(Wc):
    """Offset -> slot number of the 2x2 window {0, 1, Wc, Wc + 1} (None: no slot)."""
    return {0: 0, 1: 1, Wc: 2, Wc + 1: 3}.get


def decode_window(ptr, off, val, nslots, slot_of):
    """The pattern table by SLOT: (values[npat * nslots], mask[npat]) -- the value of pattern p in slot k at
    values[p * nslots + k], bit k of mask[p] set where it has one -- or None when a pattern has more than nslots entries,
    offsets that do not ascend (slot order must be storage order), an offset that is no slot, or two entries in one slot."""
    npat = len(ptr) - 1
    values = np.zeros(npat * nslots)
    mask = np.zeros(npat, dtype=np.int32)
    for p in range(npat):
        o = off[ptr[p]:ptr[p + 1]]
        if o.size > nslots or np.any(np.diff(o) <= 0):
            return None
        for j in range(ptr[p], ptr[p + 1]):
            k = slot_of(int(off[j]))
            if k is None or mask[p] & (1 << k):
                return None
            mask[p] |= 1 << k
            values[p * nslots + k] = val[j]
    return values, mask


def line_stride(off, n, radius=1):
    """The line stride W for which every offset of a square operator with n rows is a slot of the 3x3 window, or None.
    Several strides can fit (a 7-point operator {-W-1, -W, -1, 0, 1, W, W+1} also reads as a sheared stencil of stride
    W + 1): the one that cuts the rows into whole lines is preferred.
    radius 2 | 3: the same for the 5x5 | 7x7 window  c * W + d, |c|, |d| <= radius  (W >= 2 radius + 1: one reading per
    offset).  The largest offset is cy * W + dx for some 1 <= cy <= radius, |dx| <= radius: those are the candidates."""
    mx = int(np.abs(off).max()) if off.size else 0
    if mx <= 1:
        cands = [n] if n >= 3 else []                         # 1-D: one line, only the centre slots are used
    else:
        cands = []
        for cy in range(1, radius + 1):
            for dx in [0] + [s * k for k in range(1, radius + 1) for s in (1, -1)]:
                w, rem = divmod(mx - dx, cy)
                if rem == 0 and 2 * radius + 1 <= w < n and w not in cands:
                    cands.append(w)
    fits = [w for w in cands if all(_decompose(int(o), w, radius) is not None for o in off)]
    return next((w for w in fits if n % w == 0), fits[0]) if fits else None


def line_reach(off, W, radius):
    """(reach in x, reach in y): the largest |d| and |c| of the offsets  c * W + d  of a level whose offsets all fit the
    (2 radius + 1)^2 window of line stride W -- the half-bandwidths its x- and y-line systems need (at least 1)."""
    cd = [_decompose(int(o), W, radius) for o in off]
    return max([1] + [abs(d) for _, d in cd]), max([1] + [abs(c) for c, _ in cd])


def hot_pattern(cand, counts):
    """The most frequent of the candidate pattern ids `cand` (ascending; the first of equally frequent ones), -1 without
    candidates.  counts[p] = rows with pattern p: only read when there is a choice (None otherwise)."""
    if len(cand) <= 1:
        return int(cand[0]) if cand else -1
    return int(max(cand, key=lambda p: counts[p]))


def prolong_hot_pairs(p_val, p_mask, counts):
    """(pairs[2], values[9]) of a prolongation by slot (decode_window, 2x2): the usual pattern pair of an (even, odd)
    column pair on even / odd lines with exactly the slots of the tensor-product interpolation -- 0x1 | 0x3 and 0x5 | 0xF,
    id(even) | id(odd) << 8, -1 where a line parity has none -- and their 1 + 2 + 2 + 4 values in that order.
    counts[line parity][column parity][p] = rows with pattern p there.  None when a row on an even line reaches the
    coarse line below: not this shape."""
    if np.any((counts[0].sum(axis=0) > 0) & ((p_mask & 0xC) != 0)):
        return None
    pairs, pval = [], []
    for yl, want in enumerate(((0x1, 0x3), (0x5, 0xF))):
        ids = [hot_pattern([p for p in range(len(p_mask)) if p_mask[p] == want[xl] and counts[yl][xl][p] > 0], counts[yl][xl])
               for xl in range(2)]
        pairs.append(-1 if min(ids) < 0 else ids[0] | (ids[1] << 8))
        for xl in range(2):
            pval += [float(p_val[ids[xl] * 4 + k]) if ids[xl] >= 0 else 0.0 for k in range(4) if (want[xl] >> k) & 1]
    return pairs, pval


def _table(R):
    """(ptr, off, val) of a RowPatterns twin on the host."""
    return (R.pat_ptr.cpu().numpy(), R.pat_off.cpu().numpy().astype(np.int64)[: R.nent], R.pat_val.cpu().numpy()[: R.nent])


def _hot_values(values, hot):
    """The 9 slot values of pattern `hot` as a host array for the kernels' scalar registers (None: no hot pattern)."""
    return None if hot < 0 else (ctypes.c_double * 9)(*[float(v) for v in values[hot * 9: hot * 9 + 9]])


CENSUS_CELL = 32               # columns per cell of a census table (kLmgCensusCell)


def census_stride(W):
    """Row stride of the census table of a grid with line stride W: its cells and the border column."""
    return (int(W) + CENSUS_CELL - 1) // CENSUS_CELL + 1


def census_table(pid, n, W, expected):
    """The census (lmg_pattern_census, include/lmg.h) of the rows of the id array `pid` -- n rows in lines of W -- that do
    not hold the id expected[2 * (line & 1) + (column & 1)]: int32 2-D prefix sums over (line, cell of 32 columns), from
    which the register-fused passes read which waves meet nothing but hot rows.  Built by the twin that decides the hot
    ids, next to them, from the ids it holds: a table lives and dies with its twin, and a twin is never changed in place
    (DeviceCSR.pack / repack_values build new ones), so it cannot go stale.  None when any expected id is missing, and for
    ids that are not on a device (the passes then run without)."""
    if min(expected) < 0 or not pid.is_cuda:
        return None
    L = _lib.lib()
    count = int(L.lmg_pattern_census_count(int(n), int(W)))
    if count <= 0:
        return None
    table = torch.empty(count, dtype=I32, device=pid.device)
    exp = (ctypes.c_int32 * 4)(*[int(e) for e in expected])
    check(L.lmg_pattern_census(int(n), int(W), _p(pid), ctypes.addressof(exp), _p(table), _s(pid)), "lmg_pattern_census")
    return table


class PackedCSR:
    """Lossless packed twin of a DeviceCSR for lmg_pcsr_sweep (see include/lmg.h):
    uint8 row lengths, uint16 tile-relative columns when every 512-row tile spans < 65536
    columns, and a value dictionary (uint8 / uint16 indices) when the matrix has few
    distinct values -- compared BITWISE, so -0.0 / NaN payloads survive.  Built at setup by the
    kernels of csrc/pack.hip (format conversion, like SciPy's csc -> csr)."""

    __slots__ = ("n", "nnz", "shape", "tile_rows", "tile_cap", "tile_base", "tile_colbase", "rowlen", "col",
                 "colmode", "val", "valmode", "dict", "ndict", "bytes_")

    @staticmethod
    def _padded(t):
        raw = t.contiguous().view(torch.uint8)
        out = torch.zeros(((raw.numel() + 15) // 16) * 16 + 16, dtype=torch.uint8, device=t.device)
        out[: raw.numel()] = raw
        return out

    _VSET_SLOTS = 1 << 20          # uint64 slots of the distinct-value table (8 MB)
    _VSET_LIMIT = 65536            # more distinct values than this: raw fp64 stream

    @staticmethod
    def _padded_empty(nbytes, device):
        return torch.zeros(((nbytes + 15) // 16) * 16 + 16, dtype=torch.uint8, device=device)

    @classmethod
    def _distinct_values(cls, vals, limit=None):
        """Sorted (as signed 64-bit patterns) distinct values of `vals`, or None when there are
        more than `limit` (default _VSET_LIMIT) of them.  Hash-set kernel + a sort of the few
        survivors instead of sorting all nnz values."""
        L = _lib.lib()
        dev = vals.device
        limit = cls._VSET_LIMIT if limit is None else int(limit)
        table = torch.full((cls._VSET_SLOTS,), -1, dtype=torch.int64, device=dev)
        state = torch.zeros(4, dtype=I32, device=dev)
        check(L.lmg_value_set_insert(vals.numel(), _p(vals), _p(table), cls._VSET_SLOTS, limit,
                                     _p(state), _s(vals)), "lmg_value_set_insert")
        st = state.cpu()
        if int(st[1]):
            return None
        # the few survivors: collected by an own kernel, sorted on the host (a library sort / mask / cat each cost
        # 50 - 75 ms of code-object loading in a fresh process)
        cap = limit + 8
        out = torch.empty(cap, dtype=torch.int64, device=dev)
        cnt = torch.zeros(1, dtype=I32, device=dev)
        check(L.lmg_value_set_collect(_p(table), cls._VSET_SLOTS, _p(out), cap, _p(cnt), _s(vals)), "lmg_value_set_collect")
        k = int(cnt.cpu()[0])
        if k > cap:
            return None
        keys = out[:k].cpu().numpy()
        if int(st[2]):
            keys = np.concatenate([keys, np.array([-1], dtype=np.int64)])
        if keys.size > limit:
            return None
        return torch.from_numpy(np.sort(keys)).to(dev)

    @staticmethod
    def _encode_values(vals, uniq, width, out):
        missing = torch.zeros(1, dtype=I32, device=vals.device)
        check(_lib.lib().lmg_value_encode(vals.numel(), _p(vals), _p(uniq), int(uniq.numel()), width, _p(out),
                                          _p(missing), _s(vals)), "lmg_value_encode")
        if int(missing):
            raise LmgError("value dictionary does not cover the matrix values")

    @classmethod
    def from_csr(cls, A, tile_rows=None, colmode=None):
        """tile_rows (512, 128 or 64) and colmode (0: uint16 tile-relative columns, 1: int32) override the choices made
        below -- the format allows any tile height and int32 columns for any matrix; None keeps the builder's own rule.
        The value encoding always follows from the number of distinct values.  (pack() passes neither: the parity tests
        reach the short tiles and the int32 columns on small matrices this way.)"""
        n, nnz = A.shape[0], A.nnz
        if n == 0 or nnz == 0:
            return None
        if tile_rows is not None and int(tile_rows) not in (512, 128, 64):
            raise ValueError("tile_rows must be 512, 128 or 64, got %r" % (tile_rows,))
        if colmode is not None and int(colmode) not in (0, 1):
            raise ValueError("colmode must be 0 or 1, got %r" % (colmode,))
        L = _lib.lib()
        dev = A.vals.device
        rowlen = (A.rowptr[1:] - A.rowptr[:-1])
        if int(rowlen.max()) > 255 or int(rowlen.min()) < 0:
            return None
        # value encoding first: it decides how many bytes an entry occupies in LDS
        uniq = cls._distinct_values(A.vals)
        ndict = int(uniq.numel()) if uniq is not None else 1 << 30
        # tile height: 512 rows unless the rows are so long that a tile would not leave room for
        # several workgroups per CU (budget ~20 KB of LDS per tile); long-row tiles only exist
        # for the VAL8 / VAL64 encodings
        avg = nnz / n
        T = int(L.lmg_pcsr_tile_rows())
        bpe = 2 + (1 if ndict <= 256 else (2 if ndict <= 65536 else 8))
        if tile_rows is not None:
            T = int(tile_rows)
        elif T * avg * bpe > 20480:
            T = 128 if 128 * avg * (2 + (1 if ndict <= 256 else 8)) <= 20480 else 64
            if 256 < ndict <= 65536:
                ndict = 1 << 30                    # force raw values
        ntile = (n + T - 1) // T
        tb = A.rowptr[0:n:T]
        tile_base = torch.cat([tb, A.rowptr[n:n + 1]]).contiguous()
        tile_nnz = tile_base[1:] - tile_base[:-1]
        self = cls()
        self.n, self.nnz, self.shape = n, nnz, A.shape
        self.tile_rows = T
        self.tile_cap = int(tile_nnz.max())
        self.tile_base = tile_base
        self.rowlen = rowlen.to(torch.uint8).contiguous()
        cmin = torch.empty(ntile, dtype=I32, device=dev)
        cmax = torch.empty(ntile, dtype=I32, device=dev)
        check(L.lmg_pcsr_tile_colrange(n, T, _p(A.rowptr), _p(A.colidx), _p(cmin), _p(cmax), _s(A.rowptr)),
              "lmg_pcsr_tile_colrange")
        self.tile_colbase = cmin
        fits16 = int((cmax - cmin).max()) < 65536
        if colmode == 0 and not fits16:
            raise ValueError("colmode 0: a tile spans 65536 columns or more")
        if (fits16 if colmode is None else int(colmode) == 0):
            self.colmode = 0
            self.col = cls._padded_empty(2 * nnz, dev)
            check(L.lmg_pcsr_encode_cols16(n, T, _p(A.rowptr), _p(A.colidx), _p(cmin), _p(self.col), _s(A.rowptr)),
                  "lmg_pcsr_encode_cols16")
        else:
            self.colmode = 1
            self.col = cls._padded(A.colidx)
        self.ndict = ndict
        if self.ndict <= 256:
            self.valmode = 0
            self.val = cls._padded_empty(nnz, dev)
            cls._encode_values(A.vals, uniq, 1, self.val)
            self.dict = uniq.view(F64)
        elif self.ndict <= 65536:
            self.valmode = 1
            self.val = cls._padded_empty(2 * nnz, dev)
            cls._encode_values(A.vals, uniq, 2, self.val)
            self.dict = uniq.view(F64)
        else:
            self.valmode = 2
            self.val = cls._padded(A.vals)
            self.dict = None
            self.ndict = 0
        self.bytes_ = (self.rowlen.numel() + 8 * ntile + nnz * ((2, 4)[self.colmode] + (1, 2, 8)[self.valmode]))
        return self

    def bytes(self):
        return int(self.bytes_)

    def sweep_args(self):
        """The arguments of lmg_pcsr_sweep between the mode and the vectors, and the tensor whose stream it takes."""
        return (self.n, self.nnz, self.tile_rows, self.tile_cap, _p(self.tile_base), _p(self.tile_colbase), _p(self.rowlen),
                _p(self.col), self.colmode, _p(self.val), self.valmode, _p(self.dict), self.ndict), self.tile_base

    def update_values(self, A):
        """New values, same sparsity pattern (Galerkin rebuild): only the value stream (and the
        dictionary) is re-encoded; returns False when the value encoding no longer fits and the
        caller has to repack from scratch."""
        if A.nnz != self.nnz:
            return False
        if self.valmode == 2:
            self.val[: self.nnz * 8].view(F64).copy_(A.vals)
            return True
        uniq = self._distinct_values(A.vals)
        nd = int(uniq.numel()) if uniq is not None else 1 << 30
        if (self.valmode == 0 and nd > 256) or (self.valmode == 1 and nd > 65536):
            return False
        self._encode_values(A.vals, uniq, 1 if self.valmode == 0 else 2, self.val)
        self.dict = uniq.view(F64)
        self.ndict = nd
        return True


class SellCSR:
    """Sliced-ELL (SELL-64) twin of a DeviceCSR for lmg_sell_sweep (see include/lmg.h): slices of 64
    rows padded to their longest row, entries stored column-major inside a slice.  For long rows
    with all-distinct values (Galerkin operators of learned / L2-type transfers); refused when the
    padding would cost more than 20 % extra entries.
    values "f32": the value stream is fp32 and the twin represents A32 = double(float(A)) value by value
    (lmg_sell_sweep_f32: a cycle used as a preconditioner); refused -- None -- when a stored value other than 0 is not
    finite or rounds to +-inf, a subnormal or zero."""

    __slots__ = ("n", "nnz", "shape", "slice_base", "slice_len", "slice_cmin", "rowlen", "col", "colmode", "val",
                 "max_len", "padded", "bytes_", "values")

    MAX_PADDING = 1.2

    @classmethod
    def from_csr(cls, A, colmode=None, max_padding=None, values="f64"):
        """colmode (0: uint16 slice-relative columns, 1: int32) and max_padding (padded entries per entry of the matrix
        from which the twin is refused; default MAX_PADDING) override the choices made below -- the format allows int32
        columns and any padding for any matrix; None keeps the builder's own rule.  (pack() passes neither: the parity
        tests reach the int32 columns and ragged slices on small matrices this way.)"""
        check_values(values)
        n, nnz = A.shape[0], A.nnz
        if n == 0 or nnz == 0 or not A.vals.is_cuda:
            return None
        if colmode is not None and int(colmode) not in (0, 1):
            raise ValueError("colmode must be 0 or 1, got %r" % (colmode,))
        L = _lib.lib()
        dev = A.vals.device
        nsl = (n + 63) // 64
        slice_len = torch.empty(nsl, dtype=I32, device=dev)
        cmin = torch.empty(nsl, dtype=I32, device=dev)
        cmax = torch.empty(nsl, dtype=I32, device=dev)
        check(L.lmg_sell_slice_info(n, _p(A.rowptr), _p(A.colidx), _p(slice_len), _p(cmin), _p(cmax), _s(A.rowptr)),
              "lmg_sell_slice_info")
        padded = 64 * int(slice_len.long().sum())
        if padded > (cls.MAX_PADDING if max_padding is None else max_padding) * nnz or padded >= 2 ** 31 - 64:
            return None
        self = cls()
        self.n, self.nnz, self.shape, self.padded = n, nnz, A.shape, padded
        sl = slice_len.long() * 64
        self.slice_base = (torch.cumsum(sl, 0) - sl).contiguous()
        self.slice_len = slice_len
        self.slice_cmin = cmin
        self.rowlen = (A.rowptr[1:] - A.rowptr[:-1]).contiguous()
        self.max_len = int(slice_len.max())
        fits16 = int((cmax - cmin).max()) < 65536
        if colmode == 0 and not fits16:
            raise ValueError("colmode 0: a slice spans 65536 columns or more")
        self.colmode = (0 if fits16 else 1) if colmode is None else int(colmode)
        self.col = torch.zeros(padded + 64, dtype=torch.int16 if self.colmode == 0 else I32, device=dev)
        self.values = values
        self.val = torch.zeros(padded + 64, dtype=F64 if values == "f64" else F32, device=dev)
        if not self._fill(A, self.col):
            return None
        self.bytes_ = padded * ((2, 4)[self.colmode] + self.val.element_size()) + 16 * nsl + 4 * n
        return self

    def _fill(self, A, col):
        """The value stream (and with `col` the columns) from A; False when fp32 values fail the range rule."""
        L = _lib.lib()
        head = (self.n, _p(A.rowptr), None if col is None else _p(A.colidx), _p(A.vals), _p(self.slice_base),
                _p(self.slice_cmin), self.colmode, _p(col), _p(self.val))
        if self.values == "f64":
            check(L.lmg_sell_fill(*head, _s(A.rowptr)), "lmg_sell_fill")
            return True
        flag = torch.zeros(1, dtype=I32, device=self.val.device)
        check(L.lmg_sell_fill_f32(*head, _p(flag), _s(A.rowptr)), "lmg_sell_fill_f32")
        return not int(flag.cpu()[0])

    def bytes(self):
        return int(self.bytes_)

    def sweep_args(self):
        """The arguments of lmg_sell_sweep between the mode and the vectors, and the tensor whose stream it takes."""
        return (self.n, _p(self.slice_base), _p(self.slice_len), _p(self.slice_cmin), _p(self.rowlen), _p(self.col),
                self.colmode, _p(self.val), self.max_len), self.slice_base

    def update_values(self, A):
        """New values, same pattern (Galerkin rebuild): only the value stream is rewritten, at the width it has.  False
        when fp32 values fail the range rule (the caller rebuilds the twin in fp64)."""
        return self._fill(A, None)


class ColorSell:
    """The matrix in the order of a colour schedule, sliced-ELL as SellCSR, for lmg_color_sweep (see include/lmg.h): every
    colour starts on a slice boundary -- its last slice is filled up with empty rows, id -1 --, slice s is padded to its
    longest row, entry j of scheduled row k lives at slice_base[s] + 64 j + (k mod 64).  int32 columns, fp64 copies of the
    values, and per entry its index in A.vals (`src`, -1 for padding) for update_values.  Built on the device from the
    schedule's row list (count, scan, fill); the host only handles the per-colour pointers."""

    __slots__ = ("n", "ncolors", "nslices", "h_color_slice", "trow", "tlen", "slice_len", "slice_base", "col", "val", "src",
                 "max_len", "padded", "key")

    @classmethod
    def from_schedule(cls, A, d_rows, h_ptr):
        """d_rows: the rows ordered by (colour, row) on A's device; h_ptr: the host pointers of the colours into it."""
        L = _lib.lib()
        dev = A.vals.device
        self = cls()
        self.n = A.shape[0]
        self.key = (A.rowptr.data_ptr(), A.colidx.data_ptr(), A.nnz)
        h_ptr = np.ascontiguousarray(h_ptr, dtype=np.int32)
        self.ncolors = nc = int(h_ptr.size - 1)
        self.h_color_slice = np.zeros(nc + 1, dtype=np.int32)
        np.cumsum((np.diff(h_ptr) + 63) // 64, out=self.h_color_slice[1:])
        self.nslices = nsl = int(self.h_color_slice[-1])
        self.trow = torch.empty(max(64 * nsl, 1), dtype=I32, device=dev)
        self.tlen = torch.empty(max(64 * nsl, 1), dtype=I32, device=dev)
        self.slice_len = torch.empty(max(nsl, 1), dtype=I32, device=dev)
        if nsl == 0:
            self.slice_base = torch.zeros(1, dtype=torch.int64, device=dev)
            self.max_len = self.padded = 0
            self.col, self.src = (torch.zeros(64, dtype=I32, device=dev) for _ in range(2))
            self.val = torch.zeros(64, dtype=F64, device=dev)
            return self
        d_ptr = torch.from_numpy(h_ptr).to(dev)
        d_cs = torch.from_numpy(self.h_color_slice).to(dev)
        check(L.lmg_color_twin_count(nsl, nc, _p(d_ptr), _p(d_cs), _p(d_rows), _p(A.rowptr), _p(self.trow), _p(self.tlen),
                                     _p(self.slice_len), _s(A.rowptr)), "lmg_color_twin_count")
        sl = self.slice_len.long() * 64
        ends = torch.cumsum(sl, 0)
        self.slice_base = (ends - sl).contiguous()
        self.padded, self.max_len = (int(v) for v in torch.stack((ends[-1], self.slice_len.max().long())).cpu())
        self.col = torch.zeros(self.padded + 64, dtype=I32, device=dev)
        self.val = torch.zeros(self.padded + 64, dtype=F64, device=dev)
        self.src = torch.full((self.padded + 64,), -1, dtype=I32, device=dev)
        entries = A.colidx if A.nnz else torch.zeros(1, dtype=I32, device=dev)      # (no row has entries then)
        values = A.vals if A.nnz else torch.zeros(1, dtype=F64, device=dev)
        check(L.lmg_color_twin_fill(nsl, _p(self.trow), _p(A.rowptr), _p(entries), _p(values), _p(self.slice_base),
                                    _p(self.col), _p(self.val), _p(self.src), _s(A.rowptr)), "lmg_color_twin_fill")
        return self

    def update_values(self, A):
        """New values, same pattern (Galerkin rebuild): the value stream again from the source indices."""
        if self.padded and A.nnz:
            check(_lib.lib().lmg_color_twin_refill(self.padded, _p(self.src), _p(A.vals), _p(self.val), _s(A.vals)),
                  "lmg_color_twin_refill")

    def bytes(self):
        return 16 * self.padded + 12 * self.nslices + 8 * 64 * self.nslices

    def sweep(self, x, b, sweeps, backward):
        check(_lib.lib().lmg_color_sweep(self.ncolors, self.h_color_slice.ctypes.data, _p(self.slice_base), _p(self.slice_len),
                                         _p(self.trow), _p(self.tlen), _p(self.col), _p(self.val), self.max_len, self.padded,
                                         _p(x), _p(b), int(sweeps), int(bool(backward)), _s(x)), "lmg_color_sweep")


def _pid_counts(R):
    """How often every pattern id of a RowPatterns twin occurs (own histogram kernel: a library one costs 0.4 s of
    code-object loading in a fresh process)."""
    cnt = torch.zeros(4 * 256, dtype=I32, device=R.pid.device)
    check(_lib.lib().lmg_pattern_parity_counts(int(R.n), 1, _p(R.pid), _p(cnt), _s(R.pid)), "lmg_pattern_parity_counts")
    return cnt.cpu().numpy().reshape(4, 256).sum(axis=0)[:R.npat].astype(np.int64)


class RowPatterns:
    """Lossless row-pattern twin of a DeviceCSR for lmg_rpat_sweep (see include/lmg.h): every
    distinct row -- (length; column - row and value bits of each entry, in storage order) -- is
    stored once, each row carries a uint8 pattern id.  Only matrices with at most 255 distinct
    rows and 1024 pattern entries qualify (assembled constant-coefficient grid operators and
    their Galerkin coarsenings); from_csr returns None for everything else."""

    __slots__ = ("n", "nnz", "shape", "pid", "npat", "nent", "max_len", "pat_ptr", "pat_off", "pat_val", "bytes_",
                 "grid_map", "_gm")

    @staticmethod
    def grid_map_candidates(shape, line_strides=None):
        """Column-base maps worth trying for a RECTANGULAR operator (see lmg_rpat_sweep_grid): the
        tensor-product transfer between two square grids when both dimensions are perfect squares, and
        the 1-D transfer.  line_strides = (fine, coarse) line lengths of a transfer between blocks of whole grid
        lines that are not square (the local blocks of a distributed level): tried first.  Nothing is assumed: a
        map is only used if every entry verifies."""
        nr, nc = int(shape[0]), int(shape[1])
        if nr == nc or nr < 2 or nc < 2:
            return []
        out = []
        if line_strides is not None:
            wf, wcs = int(line_strides[0]), int(line_strides[1])
            if wf >= 2 and wcs >= 2:
                out.append((wf, wcs, 1, 1, 0) if nr > nc else (wcs, 2 * wf, 0, 0, 1))
        wr, wc = math.isqrt(nr), math.isqrt(nc)
        if wr * wr == nr and wc * wc == nc and min(wr, wc) >= 2:
            out.append((wr, wc, 1, 1, 0) if nr > nc else (wr, 2 * wc, 0, 0, 1))
        out.append((nr + 1, 0, 0, 1, 0) if nr > nc else (nr + 1, 0, 0, 0, 1))
        return out

    @staticmethod
    def grid_base(grid_map, rows):
        """base(row) of lmg_rpat_sweep_grid for an int64 numpy array of rows."""
        if grid_map is None:
            return rows
        rl, cs, ysh, xsh, xshl = grid_map
        y, x = rows // rl, rows % rl
        return (y >> ysh) * cs + ((x >> xsh) << xshl)

    @classmethod
    def from_csr(cls, A, grid_map=None):
        n, nnz = A.shape[0], A.nnz
        if n == 0 or nnz == 0 or not A.vals.is_cuda:
            return None
        L = _lib.lib()
        dev = A.vals.device
        gm = None if grid_map is None else (ctypes.c_int32 * 5)(*[int(v) for v in grid_map])
        gmp = None if gm is None else ctypes.addressof(gm)
        mp, me = ctypes.c_int32(0), ctypes.c_int32(0)
        check(L.lmg_rpat_limits(ctypes.addressof(mp), ctypes.addressof(me)), "lmg_rpat_limits")
        max_pat, max_ent = int(mp.value), int(me.value)
        hashes = torch.empty(n, dtype=torch.int64, device=dev)
        check(L.lmg_rpat_row_hash_grid(n, gmp, _p(A.rowptr), _p(A.colidx), _p(A.vals), _p(hashes), _s(A.rowptr)),
              "lmg_rpat_row_hash_grid")
        uniq = PackedCSR._distinct_values(hashes.view(F64), limit=max_pat)
        if uniq is None:
            return None
        npat = int(uniq.numel())
        # (32 spare bytes behind the ids: the LDS-staged Gauss-Seidel bands fetch them in aligned dwords, up to 19 bytes past n)
        pid = torch.zeros(n + 32, dtype=torch.uint8, device=dev)[:n]
        PackedCSR._encode_values(hashes.view(F64), uniq, 1, pid)
        del hashes
        rep = torch.full((256,), -1, dtype=I32, device=dev)
        check(L.lmg_rpat_claim(n, _p(pid), _p(rep), _s(pid)), "lmg_rpat_claim")
        # (the pattern table is a few hundred numbers: index gathers on the device, the arithmetic on the host -- every
        # library elementwise kernel used for the first time costs 50 - 75 ms of code-object loading)
        rep_h = rep[:npat].cpu().numpy().astype(np.int64)
        if npat == 0 or rep_h.min() < 0:
            return None
        rep = torch.from_numpy(rep_h).to(dev)
        starts, ends = A.rowptr[rep].cpu().numpy().astype(np.int64), A.rowptr[torch.from_numpy(rep_h + 1).to(dev)].cpu().numpy().astype(np.int64)
        lens = ends - starts
        nent = int(lens.sum())
        if nent > max_ent:
            return None
        idx = np.concatenate([np.arange(s_, e_) for s_, e_ in zip(starts, ends)]) if nent else np.zeros(0, np.int64)
        d_idx = torch.from_numpy(idx).to(dev)
        self = cls()
        self.n, self.nnz, self.shape = n, nnz, A.shape
        self.pid = pid
        self.npat, self.nent = npat, nent
        self.max_len = int(lens.max())
        ptr = np.zeros(npat + 1, dtype=np.int32)
        np.cumsum(lens, out=ptr[1:])
        self.pat_ptr = torch.from_numpy(ptr).to(dev)
        base_of = cls.grid_base(grid_map, np.repeat(rep_h, lens).astype(np.int64))
        if nent:
            off_h = A.colidx[d_idx].cpu().numpy().astype(np.int64) - base_of
            if np.abs(off_h).max() >= 2 ** 31:
                return None
            self.pat_off = torch.from_numpy(off_h.astype(np.int32)).to(dev)
        else:
            self.pat_off = torch.zeros(1, dtype=I32, device=dev)
        self.pat_val = A.vals[d_idx].contiguous() if nent else torch.zeros(1, dtype=F64, device=dev)
        mismatch = torch.zeros(1, dtype=I32, device=dev)
        check(L.lmg_rpat_verify_grid(n, A.shape[1], gmp, _p(A.rowptr), _p(A.colidx), _p(A.vals), _p(pid), npat,
                                     _p(self.pat_ptr), _p(self.pat_off), _p(self.pat_val), _p(mismatch), _s(A.rowptr)),
              "lmg_rpat_verify_grid")
        if int(mismatch):
            return None                                # a hash collision: not worth a second try
        self.bytes_ = n + 4 * (npat + 1) + 12 * nent
        self.grid_map = None if grid_map is None else tuple(int(v) for v in grid_map)
        self._gm = gm                                  # keeps the host array of the map alive
        return self

    def bytes(self):
        return int(self.bytes_)

    def sweep_args(self):
        """The arguments of lmg_rpat_sweep_grid between the mode and the vectors, and the tensor whose stream it takes."""
        gmp = None if self._gm is None else ctypes.addressof(self._gm)
        return (self.n, gmp, _p(self.pid), self.npat, self.nent, self.max_len, _p(self.pat_ptr), _p(self.pat_off),
                _p(self.pat_val)), self.pid


class StencilTwin:
    """3x3-stencil view of a RowPatterns twin for lmg_stencil_sweep (see include/lmg.h): every entry
    of every pattern at  column - row = c * W + d,  c, d in {-1, 0, 1},  for ONE line stride W, every
    pattern in ascending column order.  Derived from the (already verified) pattern table on the host
    -- a few hundred numbers --; the per-row pattern ids are shared with the RowPatterns twin.
    from_patterns returns None for everything that does not fit (the RPAT kernel then runs)."""

    __slots__ = ("n", "W", "npat", "pid", "st_val", "st_mask", "umask", "bytes_", "patterns", "hot", "_hot_val",
                 "_gs_ok", "_gs_work", "_line_end", "census")
    _decompose = staticmethod(_decompose)

    @classmethod
    def from_patterns(cls, R, shape):
        if R is None or shape[0] != shape[1] or R.n < 2:
            return None
        mp = ctypes.c_int32(0)
        check(_lib.lib().lmg_stencil_limits(ctypes.addressof(mp)), "lmg_stencil_limits")
        if R.npat > int(mp.value):
            return None
        ptr, off, val = _table(R)
        W = line_stride(off, int(R.n))
        dec = None if W is None else decode_window(ptr, off, val, 9, slot_3x3(W))
        if dec is None:
            return None
        st_val, st_mask = dec
        dev = R.pid.device
        self = cls()
        self.n, self.W, self.npat, self.pid, self.patterns = int(R.n), int(W), int(R.npat), R.pid, R
        self.st_val = torch.from_numpy(st_val).to(dev)
        self.st_mask = torch.from_numpy(st_mask).to(dev)
        self.umask = int(np.bitwise_or.reduce(st_mask)) if R.npat else 0
        self.bytes_ = R.n + 76 * R.npat
        # hot pattern for the fused smoothing pass: the most frequent one among those that have every
        # union slot and a non-zero diagonal (the interior row of a grid operator)
        cand = [p for p in range(R.npat) if st_mask[p] == self.umask and (st_mask[p] & 16) and st_val[p * 9 + 4] != 0.0]
        self.hot = hot_pattern(cand, _pid_counts(R) if len(cand) > 1 else None)
        self._hot_val = _hot_values(st_val, self.hot)
        # where the rows are that are NOT the hot one: the register pass runs its id-free body everywhere else
        self.census = None
        if self.hot >= 0 and _lib.lib().lmg_stencil_smooth_supported(self.umask):
            self.census = census_table(R.pid, self.n, self.W, [self.hot] * 4)
        # (bytes() stays what a sweep over the twin moves -- bench.py reads it as that --: no sweep reads the table, one wave
        # of a fused pass four words of it.  The tables are counted in Hierarchy.twin_bytes)
        # wavefront Gauss-Seidel (lmg_stencil_gs_sweep): see gs_ok below (decided on first use)
        self._gs_work = None
        self._gs_ok = None
        self._line_end = None
        return self

    def sweep_args(self):
        """The arguments of lmg_stencil_sweep between the mode and the vectors, and the tensor whose stream it takes."""
        return (self.n, self.W, _p(self.pid), self.npat, _p(self.st_val), _p(self.st_mask), self.umask), self.pid

    def c_args(self):
        """The nine leading arguments that describe this operator to lmg_stencil_smooth* / lmg_stencil_gs_sweep*."""
        hv = None if self._hot_val is None else ctypes.addressof(self._hot_val)
        return (self.n, self.W, _p(self.pid), self.npat, _p(self.st_val), _p(self.st_mask), self.umask, self.hot, hv)

    @property
    def gs_ok(self):
        """Whether the wavefront Gauss-Seidel kernel may run on this operator: a supported slot set and no coupling
        across the ends of a line -- rows in column 0 must not reach column - 1, rows in column W - 1 not column + 1.
        Decided on first use (a few library elementwise kernels on the ids of two grid columns: their code objects
        cost 0.13 s to load in a fresh process, which a Jacobi-only run never needs).
        (1-D chains are one lane of the wavefront kernel; the one-wave chain executor of gs.hip, x in LDS, is
        faster there: 0.29 vs 0.5 us per row)"""
        if self._gs_ok is None:
            ok = bool(_lib.lib().lmg_stencil_gs_supported(self.umask)) and self.n >= 2 and bool(self.umask & 0x1C7)
            self._gs_ok = ok and not self.line_end_coupling
        return self._gs_ok

    @property
    def line_end_coupling(self):
        """Whether an entry crosses the end of a line: a row in column 0 with a slot of column - 1 (0, 3, 6), or a row in
        column W - 1 with a slot of column + 1 (2, 5, 8) -- x-periodic operators, 7-point operators read with the stride of
        their other orientation.  The sweeps and the plain fused passes are linear in the row index and take such an
        operator; what finds a neighbour by grid line does not (gs_ok; the transfers folded into the register pass, whose
        lanes own coarse columns).  Decided on first use, for the reason given at gs_ok."""
        if self._line_end is None:
            mk = self.st_mask.cpu().numpy()
            W = self.W
            first = mk[self.pid[0::W].cpu().numpy()]
            last = mk[self.pid[W - 1::W].cpu().numpy()]
            self._line_end = bool(((first & 0x49) != 0).any()) or bool(((last & 0x124) != 0).any())
        return self._line_end

    def bytes(self):
        return int(self.bytes_)


class ProlongTwin:
    """2x2-window view of the row-pattern twin of a PROLONGATION between nested grids for
    lmg_stencil_smooth_prolong (see include/lmg.h): row (y, x) of the fine grid (line stride W) reads the coarse
    vector only at ((y >> 1) * Wc + (x >> 1)) + {0, 1, Wc, Wc + 1} -- the tensor-product interpolation of
    Multigrid.interpolator applied along both axes.  Derived on the host from the (already verified) pattern
    table of a RowPatterns twin with the column-base map (W, Wc, 1, 1, 0); from_patterns returns None for
    everything else (the correction then runs as its own lmg_rpat_sweep_grid launch)."""

    __slots__ = ("n", "W", "nc", "Wc", "npat", "pid", "p_val", "p_mask", "_hot_pairs", "_hot_pval", "patterns", "census")

    @classmethod
    def from_patterns(cls, R, shape):
        if R is None or R.grid_map is None or R.npat > 64 or R.n < 2:
            return None
        W, Wc, ysh, xsh, xshl = R.grid_map
        if (ysh, xsh, xshl) != (1, 1, 0) or Wc < 2 or W < 3 or 2 * Wc < W + 1 or shape[1] >= 2 ** 31:
            return None
        dec = decode_window(*_table(R), 4, slot_2x2(Wc))
        if dec is None:
            return None
        p_val, p_mask = dec
        dev = R.pid.device
        # which patterns occur where: counts by (line parity, column parity)
        n = int(R.n)
        cnt = torch.zeros(4 * 256, dtype=I32, device=dev)
        check(_lib.lib().lmg_pattern_parity_counts(n, int(W), _p(R.pid), _p(cnt), _s(R.pid)), "lmg_pattern_parity_counts")
        counts = cnt.cpu().numpy().reshape(2, 2, 256)[:, :, :R.npat].astype(np.int64)
        hot = prolong_hot_pairs(p_val, p_mask, counts)
        if hot is None:
            return None
        self = cls()
        self.n, self.W, self.nc, self.Wc, self.npat = n, int(W), int(shape[1]), int(Wc), int(R.npat)
        self.pid, self.patterns = R.pid, R
        self.p_val = torch.from_numpy(p_val).to(dev)
        self.p_mask = torch.from_numpy(p_mask).to(dev)
        # (the values of the hot pairs travel in scalar registers)
        self._hot_pairs = (ctypes.c_int32 * 2)(*hot[0])
        self._hot_pval = (ctypes.c_double * 9)(*hot[1])
        # rows that are not the hot pair's pattern for their (line parity, column parity); no table without both pairs
        pe, po = hot[0]
        self.census = census_table(R.pid, n, W, [-1] * 4 if min(pe, po) < 0 else [pe & 255, pe >> 8, po & 255, po >> 8])
        return self

    def c_args(self, e):
        """The arguments that describe the correction P e to the lmg_stencil_smooth*_prolong / _turnaround entry points."""
        return (self.nc, self.Wc, _p(e), _p(self.pid), self.npat, _p(self.p_val), _p(self.p_mask),
                ctypes.addressof(self._hot_pairs), ctypes.addressof(self._hot_pval))


class RestrictTwin:
    """3x3-window view of the row-pattern twin of a RESTRICTION between nested grids for
    lmg_stencil_smooth_restrict (see include/lmg.h): row (Y, X) of the coarse grid (line stride Wc) reads the
    fine vector (line stride W) only at (2 Y * W + 2 X) + c * W + d, c, d in {-1, 0, 1} -- the transpose of the
    tensor-product interpolation.  Derived on the host from the pattern table of a RowPatterns twin with the
    column-base map (Wc, 2 W, 0, 0, 1); None for everything else (the restriction then is its own launch)."""

    __slots__ = ("nc", "Wc", "n", "W", "npat", "pid", "r_val", "r_mask", "hot", "_hot_val", "patterns", "census")

    @classmethod
    def from_patterns(cls, R, shape):
        if R is None or R.grid_map is None or R.npat > 64:
            return None
        Wc, cs, ysh, xsh, xshl = R.grid_map
        if (ysh, xsh, xshl) != (0, 0, 1) or cs % 2 or Wc < 2 or shape[0] >= 2 ** 28:
            return None
        W = cs // 2
        # the fused passes write b_coarse only under fine nodes (even line, even column < W): the coarse grid must be
        # exactly that set, or rows beyond it would keep the previous cycle's right-hand side
        if W < 3 or Wc != (W + 1) // 2 or shape[1] % W or int(R.n) != ((shape[1] // W + 1) // 2) * Wc:
            return None
        dec = decode_window(*_table(R), 9, slot_3x3(W))
        if dec is None:
            return None
        r_val, r_mask = dec
        dev = R.pid.device
        self = cls()
        self.nc, self.Wc, self.n, self.W, self.npat = int(R.n), int(Wc), int(shape[1]), int(W), int(R.npat)
        self.pid, self.patterns = R.pid, R
        self.r_val = torch.from_numpy(r_val).to(dev)
        self.r_mask = torch.from_numpy(r_mask).to(dev)
        cand = [p for p in range(R.npat) if r_mask[p] == 0x1FF]
        self.hot = hot_pattern(cand, _pid_counts(R) if len(cand) > 1 else None)
        self._hot_val = _hot_values(r_val, self.hot)
        self.census = census_table(R.pid, self.nc, self.Wc, [self.hot] * 4)       # over the COARSE grid
        return self

    def c_args(self, bc):
        """The arguments that describe b_coarse = R r to the lmg_stencil_smooth*_restrict entry points (the turnaround
        pass takes them without the leading nc, Wc, which it has from the prolongation)."""
        hr = None if self._hot_val is None else ctypes.addressof(self._hot_val)
        return (self.nc, self.Wc, _p(bc), _p(self.pid), self.npat, _p(self.r_val), _p(self.r_mask), self.hot, hr)


class DiaTwin:
    """Slot arrays of a grid operator with per-row values for lmg_dia_smooth (see include/lmg.h): every entry at
    column - row = c * W + d, c, d in {-1, 0, 1}, for ONE line stride W; dia[q * n + row] = the entry of `row` in slot
    number q of the union mask (+0.0 where the row has none).  Built and verified on the device: W is guessed from a
    few rows in the middle of the matrix, a probe pass collects the slots of ALL entries for that W and refuses the
    matrix if any entry is not a slot; from_csr returns None for everything that does not fit (the packed-CSR sweeps
    then run one launch per sweep).
    values "f32": fp32 slot arrays, the twin represents A32 = double(float(A)) value by value (lmg_dia_smooth_f32);
    refused -- None -- when a stored value other than 0 is not finite or rounds to +-inf, a subnormal or zero."""

    __slots__ = ("n", "W", "umask", "nslots", "dia", "bytes_", "values")
    MIN_ROWS = 4096

    @staticmethod
    def _probe(A, W, umask, dia):
        """(flag word, slots seen) of a fill (dia: fp64 or fp32 slot arrays) or probe (dia None) pass; flag bit 0: an entry
        is no slot of the mask, bit 1 (fp32 arrays): a value fails the range rule."""
        dev = A.vals.device
        flags = torch.zeros(2, dtype=I32, device=dev)
        name = "lmg_dia_fill_f32" if dia is not None and dia.dtype == F32 else "lmg_dia_fill"
        check(getattr(_lib.lib(), name)(A.shape[0], int(W), _p(A.rowptr), _p(A.colidx), _p(A.vals), int(umask), _p(dia),
                                        flags.data_ptr(), flags.data_ptr() + 4, _s(A.rowptr)), name)
        f = flags.cpu().numpy()
        return int(f[0]), int(f[1]) & 0x1FF

    @classmethod
    def from_csr(cls, A, values="f64"):
        check_values(values)
        n = A.shape[0]
        if n < cls.MIN_ROWS or A.nnz == 0 or A.nnz > 9 * n or not A.vals.is_cuda or n >= 2 ** 31 - 4096:
            return None
        # candidate strides from the longest of a few rows in the middle: its largest |column - row| is W - 1, W or W + 1
        mid = n // 2
        rp = A.rowptr[mid:mid + 9].cpu().numpy().astype(np.int64)
        ci = A.colidx[rp[0]:rp[-1]].cpu().numpy().astype(np.int64)
        rows = np.repeat(np.arange(mid, mid + 8), np.diff(rp))
        off = np.abs(ci - rows)
        mx = int(off.max()) if off.size else 0
        if mx < 4:
            return None
        # (several strides can fit -- a 7-point operator also reads as the other 7-point orientation of stride W + 1;
        # everything is a linear index, so any of them is correct: prefer the one that cuts the rows into whole lines)
        for W in sorted((mx, mx - 1, mx + 1), key=lambda w: (n % w != 0 if w > 0 else True)):
            if not (3 <= W < n):
                continue
            bad, seen = cls._probe(A, W, 0x1FF, None)
            if bad or not (seen & 16):
                continue
            umask = next((m for m in (0x0BA, 0x1BB, 0x0FE, 0x1FF) if not (seen & ~m)), None)
            if umask is None or not _lib.lib().lmg_dia_smooth_supported(umask):
                return None
            self = cls()
            self.n, self.W, self.umask = int(n), int(W), int(umask)
            self.nslots = bin(umask).count("1")
            self.values = values
            self.dia = torch.empty(self.nslots * n, dtype=F64 if values == "f64" else F32, device=A.vals.device)
            bad, _seen = cls._probe(A, W, umask, self.dia)
            if bad:
                return None
            self.bytes_ = self.dia.element_size() * self.nslots * n
            return self
        return None

    def update_values(self, A):
        """New values on the same pattern (Galerkin rebuild of a variable-coefficient level), at the width the twin has.
        False: an entry left the pattern or -- fp32 -- a value fails the range rule."""
        bad, _seen = self._probe(A, self.W, self.umask, self.dia)
        return not bad

    def bytes(self):
        return int(self.bytes_)
