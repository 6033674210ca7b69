"""TEST-ONLY stand-in for learnmultigrid_amd.ops on CPU tensors.

It lets the -m "not gpu" suite exercise the HOST logic that sits above the kernels
(hierarchy recursion, row-block partitioning, ghost layouts, halo plans, collectives over
gloo, the Krylov loop) by routing every kernel call to the CPU oracle and the CPU twins of
the smoothers (tests/chebyshev_ref.py, tests/line_ref.py).  It lives under tests/ on purpose:
the product package never imports it and has no CPU path.

The rule of this module.  Every public function and class at module level stands for the op of
the same name in learnmultigrid_amd.ops and takes a prefix of its parameters
(tests/test_shim_signatures_cpu.py); none of them records its calls.  The module is usable as it
is (ops_mod=shim).  The package reads a name that is ABSENT as "not offered", so what the plain
stand-in does not offer must stay absent here: every stencil_* name, gs_prepare,
FUSED_MAX_SWEEPS, CapturedGraph, gemm, coarse_front and coarse_back.  Those, and everything that
records, exist only on the namespaces the three factories below return (FACTORIES; they are the
module's own tools and not part of any namespace):

    namespace(**replace)   a fresh copy of the module with an empty `calls` list
    recording_line()       ... whose line_factor / line_solve / csr_residual_norm2 / copy record
    fused(passes, ...)     ... with stand-ins of the fused passes, which record
"""
import sys as _sys
import types as _types

import numpy as np
import scipy.sparse as sp
import torch

import chebyshev_ref as _CR
import line_ref as _LR
from learnmultigrid_amd.ops import DeviceCSR, F64, I32   # pure-torch container, device agnostic
from oracle import kernels as K
from support import to_numpy as _np, to_scipy as _sp

FACTORIES = ("namespace", "recording_line", "fused")
_MAX_VECTORS = 65


def partials_count(n):
    return max(1024, (n + 255) // 256)


def _raw(A):
    """Raw CSR arrays in STORAGE order (no canonicalisation: the local matrices of the
    distributed solver keep the global entry order after their columns are renumbered)."""
    return A.shape[0], _np(A.rowptr), _np(A.colidx), _np(A.vals)


def csr_residual_norm2(A, x, b, r, partials, norm2):
    n, rp, ci, va = _raw(A)
    rr = np.empty(n)
    n2 = K.lib().orc_csr_residual(n, rp, ci, va, np.ascontiguousarray(_np(x)),
                                  np.ascontiguousarray(_np(b)[:n]), rr)
    if r is not None:
        _np(r)[:n] = rr
    if norm2 is not None:
        _np(norm2)[0] = n2


def csr_jacobi(A, x_in, b, omega, x_out):
    # rectangular local matrices (owned rows x [owned | ghosts]): the diagonal is column == row
    n, rp, ci, va = _raw(A)
    out = np.empty(n)
    K.lib().orc_csr_jacobi(n, rp, ci, va, np.ascontiguousarray(_np(x_in)),
                           np.ascontiguousarray(_np(b)[:n]), float(omega), out)
    _np(x_out)[:n] = out


def csr_spmv(A, x, y, alpha=1.0, beta=0.0):
    n, rp, ci, va = _raw(A)
    out = np.ascontiguousarray(_np(y)[:n]).copy()
    K.lib().orc_csr_spmv(n, rp, ci, va, np.ascontiguousarray(_np(x)), out, float(alpha), float(beta))
    _np(y)[:n] = out


def axpby(alpha, x, beta, y):
    yy = _np(y)
    yy[:] = alpha * _np(x) if beta == 0.0 else alpha * _np(x) + beta * yy


def vmul(alpha, x, y, out):
    _np(out)[:] = alpha * (_np(x) * _np(y))


def csr_inverse_diagonal(A):
    n, rp, ci, va = _raw(A)
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = np.zeros(n)
    on = ci == rows
    np.add.at(d, rows[on], va[on])
    out = np.zeros(n)
    np.divide(1.0, d, out=out, where=d != 0)
    return torch.from_numpy(out)


def dot(x, y, partials, out):
    _np(out)[0] = float(np.dot(_np(x), _np(y)))


def copy(src, dst):
    dst.copy_(src)


def zero(x):
    x.zero_()


def gather(idx, x, buf):
    _np(buf)[: idx.numel()] = _np(x)[_np(idx)]


def scatter(idx, buf, x):
    _np(x)[_np(idx)] = _np(buf)[: idx.numel()]


def dense_gemv(M, x, y):
    _np(y)[:] = K.dense_gemv(_np(M), _np(x))


def dense_gemv_blockdiag(M, x, y):
    k, s, _ = M.shape
    for i in range(k):
        _np(y)[i * s:(i + 1) * s] = K.dense_gemv(_np(M[i]), _np(x)[i * s:(i + 1) * s])


def dense_gemv_windows(M, x, x_stride, y, y_stride, z=None, z_stride=0, alpha=1.0):
    nb, rows, cols = M.shape
    Mn, xn, yn = _np(M), _np(x), _np(y)
    zn = None if z is None else _np(z)
    out = [(zn[k * z_stride:k * z_stride + rows] if zn is not None else 0.0)
           + alpha * K.dense_gemv(np.ascontiguousarray(Mn[k]), np.ascontiguousarray(xn[k * x_stride:k * x_stride + cols]))
           for k in range(nb)]
    for k in range(nb):
        yn[k * y_stride:k * y_stride + rows] = out[k]


def dense_gemv_windows_off(M, x, x_offsets, y, y_stride, z=None, z_stride=0, alpha=1.0):
    nb, rows, cols = M.shape
    Mn, xn, yn, off = _np(M), _np(x), _np(y), _np(x_offsets)
    zn = None if z is None else _np(z)
    out = [(zn[k * z_stride:k * z_stride + rows] if zn is not None else 0.0)
           + alpha * K.dense_gemv(np.ascontiguousarray(Mn[k]), np.ascontiguousarray(xn[off[k]:off[k] + cols]))
           for k in range(nb)]
    for k in range(nb):
        yn[k * y_stride:k * y_stride + rows] = out[k]


def coarse_front_gather(M, b, idx, y, tail_idx, tail_out):
    k, s, _ = M.shape
    bn, gi = _np(b), _np(idx)
    seg = np.where(gi >= 0, bn[np.maximum(gi, 0)], 0.0).reshape(k, s)
    for i in range(k):
        _np(y)[i * s:(i + 1) * s] = K.dense_gemv(np.ascontiguousarray(_np(M[i])), np.ascontiguousarray(seg[i]))
    _np(tail_out)[:] = bn[_np(tail_idx)]


def coarse_back_gather(W, x_tail, xidx, z, alpha, oidx, tail_idx, out, accumulate):
    k, s, cwp = W.shape
    xn, wi, zn, gi, on = _np(x_tail), _np(xidx).reshape(k, cwp), _np(z), _np(oidx), _np(out)
    for i in range(k):
        v = zn[i * s:(i + 1) * s] + alpha * K.dense_gemv(np.ascontiguousarray(_np(W[i])), np.ascontiguousarray(xn[wi[i]]))
        g = gi[i * s:(i + 1) * s]
        ok = g >= 0
        on[g[ok]] = v[ok] + on[g[ok]] if accumulate else v[ok]
    ti = _np(tail_idx)
    on[ti] = xn[:ti.size] + on[ti] if accumulate else xn[:ti.size]


def block_copy(nblocks, bs, src, src_stride, dst, dst_stride):
    sn, dn = _np(src), _np(dst)
    for k in range(nblocks):
        dn[k * dst_stride:k * dst_stride + bs] = sn[k * src_stride:k * src_stride + bs]


class SpGEMMPlan:
    def __init__(self, A, B, record="lazy"):
        self.shape = (A.shape[0], B.shape[1])

    def numeric(self, A, B, out=None):
        As, Bs = _sp(A), _sp(B)
        C = sp.csr_matrix(As @ Bs)
        C.sort_indices()
        # the pattern is the structural one, like the kernel's: SciPy drops the entries that cancel to exactly 0.0, the
        # symbolic phase of the device product keeps them as explicit zeros (csrc/spgemm.hip)
        ones = lambda M: sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
        S = sp.csr_matrix(ones(As) @ ones(Bs))
        S.sort_indices()
        key = lambda M: np.repeat(np.arange(M.shape[0], dtype=np.int64), np.diff(M.indptr)) * M.shape[1] + M.indices
        vals = np.zeros(S.nnz)
        vals[np.searchsorted(key(S), key(C))] = C.data
        C = sp.csr_matrix((vals, S.indices, S.indptr), shape=S.shape)
        new = DeviceCSR.from_scipy(C, "cpu")
        if out is not None:
            out.vals.copy_(new.vals)
            return out
        return new


class _Sched:
    """What the package reads of an ops.GSSchedule: its rows, and its kind (Hierarchy.rebuild_numeric asks every schedule of
    every level for it)."""
    kind, backward = "lexicographic", False

    def __init__(self, rows):
        self.d_rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32))


def build_gs_schedule(A_scipy_csr, kind, device):
    """The CPU stand-in executes a lexicographic schedule as what it is: the rows in ascending order."""
    if kind != "lexicographic":
        raise NotImplementedError(kind)
    return _Sched(np.arange(A_scipy_csr.shape[0], dtype=np.int32))


def csr_gs_schedule(A, x, b, sched, sweeps=1):
    n, rp, ci, va = _raw(A)
    xx = np.ascontiguousarray(_np(x))
    rows = np.sort(_np(sched.d_rows)).astype(np.int32)
    for _ in range(int(sweeps)):
        K.lib().orc_csr_gs_rows(rp, ci, va, xx, np.ascontiguousarray(_np(b)), rows, rows.size)
    _np(x)[:] = xx


def cheby_update(a, c, dinv, r, d, x, first=False):
    z = _np(dinv) * _np(r)
    dn = c * z if first else a * _np(d) + c * z
    _np(d)[:] = dn
    _np(x)[:] = _np(x) + dn


def csr_gershgorin(A, out):
    # the entries as they are stored, like the kernel: no canonicalisation (chebyshev_ref.gershgorin sorts the rows and sums
    # duplicates first, which moves |a| + |b| to |a + b| for a duplicated entry)
    n, rp, ci, va = _raw(A)
    rows = np.repeat(np.arange(n), np.diff(rp))
    asum, diag = np.zeros(n), np.zeros(n)
    np.add.at(asum, rows, np.abs(va))
    on = ci == rows
    np.add.at(diag, rows[on], va[on])
    ok = diag != 0
    _np(out)[0] = float(np.max(asum[ok] / np.abs(diag[ok]))) if ok.any() else 0.0


def line_factor(A, W, dir):
    fac, flags = _LR.factor(_sp(A), int(W), dir)
    if flags & _LR.COUPLED:
        raise ValueError("a non-zero entry couples two x-lines (an entry across the end of a line)")
    if flags & _LR.PIVOT:
        raise ValueError("a zero or non-finite pivot in the %s-line systems" % dir)
    return tuple(torch.from_numpy(v) for v in fac)


def line_solve(W, dir, first, step, fac, r, omega, x):
    xn, rn = _LR.solve(tuple(_np(v) for v in fac), int(W), dir, int(first), int(step), _np(r), float(omega), _np(x))
    _np(x)[:] = xn
    _np(r)[:] = rn


def krylov_max_vectors():
    return _MAX_VECTORS


def multi_partials_count(n, k):
    return 1024 * max(int(k), 1)


def multi_dot(V, k, w, partials, out):
    n = w.numel()
    assert V.dim() == 2 and V.is_contiguous() and 0 <= k <= min(V.shape[0], _MAX_VECTORS) and V.shape[1] >= n
    if k:
        _np(out)[:k] = _np(V)[:k, :n] @ _np(w)


def multi_axpy(V, k, coef, w, partials=None, norm2=None, subtract=True):
    n = w.numel()
    assert V.dim() == 2 and V.is_contiguous() and 0 <= k <= min(V.shape[0], _MAX_VECTORS) and V.shape[1] >= n
    ww, c = _np(w), _np(coef).copy()            # (coef may be a view of the buffer norm2 lives in)
    for j in range(k):
        ww[:] = ww - c[j] * _np(V)[j, :n] if subtract else ww + c[j] * _np(V)[j, :n]
    if norm2 is not None:
        assert partials is not None
        _np(norm2)[0] = float(ww @ ww)


# ---- namespaces: copies of the module that may offer more, and record ----------------------------------------------------
def namespace(**replace):
    """A fresh namespace with everything the module offers, an empty `calls` list, and the replacements given by keyword."""
    shim = _sys.modules[__name__]
    ns = _types.SimpleNamespace(**{k: getattr(shim, k) for k in dir(shim) if not k.startswith("__") and k not in FACTORIES})
    ns.calls = []
    vars(ns).update(replace)
    return ns


def recording_line():
    """Every line_factor / line_solve / csr_residual_norm2 / copy call is appended to ns.calls, so that a test can read the
    launch sequence of a cycle: ("factor", n, W, dir), ("solve", n, dir, first, step, omega), ("residual", n), ("copy", n)."""
    ns = namespace()

    def rec_line_factor(A, W, dir):
        ns.calls.append(("factor", A.shape[0], int(W), dir))
        return line_factor(A, W, dir)

    def rec_line_solve(W, dir, first, step, fac, r, omega, x):
        line_solve(W, dir, first, step, fac, r, omega, x)
        ns.calls.append(("solve", x.numel(), dir, int(first), int(step), float(omega)))

    def rec_csr_residual_norm2(A, x, b, r, partials, norm2):
        csr_residual_norm2(A, x, b, r, partials, norm2)
        ns.calls.append(("residual", A.shape[0]))

    def rec_copy(src, dst):
        copy(src, dst)
        ns.calls.append(("copy", src.numel()))

    ns.line_factor, ns.line_solve, ns.csr_residual_norm2, ns.copy = rec_line_factor, rec_line_solve, rec_csr_residual_norm2, rec_copy
    return ns


def _fused_pass(ns, sweep, A, x_in, b, x_out, r_out, prolong, restrict, *tag):
    """What a fused pass computes, in the order of the separate launches and in oracle arithmetic: the correction
    (prolong = (P, e)), x = sweep(A, x, b), the residual (r_out), its restriction (restrict = (R, b_coarse)); the call is
    appended to ns.calls as (kind, n) + tag."""
    assert prolong is None or restrict is None
    As = _sp(A)
    bb = _np(b)
    x = np.zeros(A.shape[0]) if x_in is None else _np(x_in).copy()
    if prolong is not None:
        x = K.spmv(_sp(prolong[0]), _np(prolong[1]), x, 1.0, 1.0)
    x = sweep(As, x, bb)
    _np(x_out)[:] = x
    r, _ = K.residual(As, x, bb)
    if r_out is not None:
        _np(r_out)[:] = r
    if restrict is not None:
        _np(restrict[1])[:] = K.matvec(_sp(restrict[0]), r)
    ns.calls.append(("prolong" if prolong is not None else "restrict" if restrict is not None else "plain", A.shape[0]) + tag)


def _product_gs_schedule(A_scipy_csr, kind, device):
    # (the product's host-side builder: colour classes and reversed() exist; the shim sweeps the rows of a schedule in
    # ascending order whatever its sets are, which is all a trace needs)
    from learnmultigrid_amd import ops
    return ops.build_gs_schedule(A_scipy_csr, kind, device)


def fused(passes="jacobi", max_rows=None, turnaround=True):
    """A namespace with stand-ins of the fused passes on matrices of at most max_rows rows (None: all); every fused call
    is recorded in ns.calls.  passes:
      "jacobi"  the Jacobi passes, recorded as (kind, n), kind in "plain" / "prolong" / "restrict"; the turnaround pass
                (the correcting pass, then the restricting pass: ("turnaround", n) in place of the two) is selected
                where `turnaround` is true
      "cheby"   the Chebyshev pass, recorded as (kind, n, degree, x_is_zero).  The Jacobi predicates exist and say yes,
                but there is no Jacobi pass and the turnaround raises: the Chebyshev cycle must not pick them up
      "all"     both, the wavefront Gauss-Seidel stand-in and the package's own build_gs_schedule (multicolour
                schedules): what the launch traces run on.  max_rows = 0: the schedules only, no fused name exists"""
    if passes not in ("jacobi", "cheby", "all"):
        raise ValueError("passes must be 'jacobi', 'cheby' or 'all', not %r" % (passes,))
    ns = namespace()
    if passes == "all":
        ns.build_gs_schedule = _product_gs_schedule
        if max_rows == 0:
            return ns
    ok = (lambda A: True) if max_rows is None else (lambda A: A.shape[0] <= max_rows)
    ns.FUSED_MAX_SWEEPS = 3
    if passes in ("cheby", "all"):
        ns.stencil_cheby_available = ok
        ns.stencil_cheby_prolong_available = lambda A, P: ok(A)
        ns.stencil_cheby_restrict_available = lambda A, R: ok(A)

        def stencil_cheby(A, x_in, b, coef, x_out, r_out=None, prolong=None, restrict=None):
            assert 1 <= len(coef) <= 3
            _fused_pass(ns, lambda As, x, bb: _CR.cheby_step(As, x, bb, coef), A, x_in, b, x_out, r_out, prolong, restrict,
                        len(coef), x_in is None)

        ns.stencil_cheby = stencil_cheby
    if passes == "cheby":
        ns.stencil_smooth_available = lambda A: True
        ns.stencil_smooth_turnaround_selected = lambda A, P, R: True

        def stencil_smooth_turnaround(A, x_in, b, omega, sweeps_post, sweeps_pre, x_out, prolong, restrict):
            raise AssertionError("the Chebyshev cycle has no turnaround pass")

        ns.stencil_smooth_turnaround = stencil_smooth_turnaround
        return ns

    def stencil_smooth(A, x_in, b, omega, sweeps, x_out, r_out=None, prolong=None, restrict=None):
        def sweep(As, x, bb):
            for _ in range(sweeps):
                x = K.jacobi(As, x, bb, omega)
            return x
        _fused_pass(ns, sweep, A, x_in, b, x_out, r_out, prolong, restrict)

    def stencil_smooth_turnaround(A, x_in, b, omega, sweeps_post, sweeps_pre, x_out, prolong, restrict):
        tmp = torch.empty_like(x_out)
        stencil_smooth(A, x_in, b, omega, sweeps_post, tmp, prolong=prolong)
        stencil_smooth(A, tmp, b, omega, sweeps_pre, x_out, restrict=restrict)
        ns.calls[-2:] = [("turnaround", A.shape[0])]

    ns.stencil_smooth, ns.stencil_smooth_turnaround = stencil_smooth, stencil_smooth_turnaround
    ns.stencil_smooth_available = ok
    ns.stencil_smooth_prolong_available = lambda A, P: ok(A)
    ns.stencil_smooth_restrict_available = lambda A, R: ok(A)
    ns.stencil_smooth_turnaround_selected = lambda A, P, R: turnaround and ok(A)
    if passes == "all":
        ns.stencil_gs_available = lambda A, direction="forward": ok(A)
        ns.stencil_gs_check = lambda A: None

        def stencil_gs(A, x, b, sweeps=1, direction="forward"):
            rows = np.flatnonzero(np.diff(_np(A.rowptr))).astype(np.int32)          # (ghost rows of a local block are empty)
            rows = rows if direction == "forward" else rows[::-1].copy()
            xx = _np(x)
            for _ in range(int(sweeps)):
                K.gs_rows(_sp(A), xx, _np(b), rows)

        ns.stencil_gs = stencil_gs
    return ns
