"""The kernels as PyTorch custom ops over ROCm tensors, `torch.ops.lmg.*` (ops.register_torch_ops() registers them), e.g.
    torch.ops.lmg.csr_jacobi(rowptr, colidx, vals, x, b, omega) -> x_new.

Stateless ops take the CSR arrays of their matrix; an operator handle (operator_create) owns a DeviceCSR with the storage
twins pack() built once (Operator), and its smoothing ops launch the sequences of smoothing.py that the solvers' cycles run."""
import types

import torch

from . import ops, smoothing
from ._lib import LmgError
from .ops import DeviceCSR, F64


class Operator:
    """What an operator handle owns: the matrix A with its twins, the inverse diagonal (built by the first two-launch
    Chebyshev step) and the Gauss-Seidel schedules per direction (built by the first sweep without a wavefront kernel).
    The smoothers launch with the ops module `o`; only those whose name ends in an underscore write the x they are given."""

    def __init__(self, A):
        self.A, self.dinv, self.gs = A, None, {}

    def jacobi(self, o, x, b, omega, sweeps):
        """x after `sweeps` weighted-Jacobi sweeps: fused passes where A has them, else one launch per sweep."""
        A, sweeps = self.A, int(sweeps)
        if sweeps <= 0:
            return x.clone()
        fused = A.stencil is not None and smoothing.ask(o, "stencil_smooth_available", A)
        v = types.SimpleNamespace(x=x, tmp=torch.empty_like(x), b=b, r=None)
        first = min(sweeps, o.FUSED_MAX_SWEEPS) if fused else 1
        for k in (first, sweeps - first):
            if k and v.tmp is x:
                v.tmp = torch.empty_like(x)      # after the first launch the spare buffer is the caller's x: never written
            if fused:
                smoothing.fused_passes(o, A, v, k, omega)
            else:
                for _ in range(k):
                    o.csr_jacobi(A, v.x, b, omega, v.tmp)
                    v.x, v.tmp = v.tmp, v.x
        return v.x

    def chebyshev(self, o, x, b, degree, lmax, ratio):
        """x after one Chebyshev step of `degree` on [lmax / ratio, lmax] (lmax <= 0: the Gershgorin bound)."""
        A = self.A
        if lmax <= 0.0:
            lmax = float(_gershgorin(o, A).item())
        coef = smoothing.chebyshev_coefficients(lmax, ratio, int(degree))
        if smoothing.ask(o, "stencil_cheby_available", A) and len(coef) <= o.FUSED_MAX_SWEEPS:
            v = types.SimpleNamespace(x=x, tmp=torch.empty_like(x), b=b, r=None)
            smoothing.fused_passes(o, A, v, len(coef), None, coef=coef)
            return v.x
        if self.dinv is None:
            self.dinv = o.csr_inverse_diagonal(A)
        v = types.SimpleNamespace(x=x.clone(), b=b, r=torch.empty_like(x), d=torch.empty_like(x), dinv=self.dinv)
        smoothing.chebyshev_step(o, A, v, coef)
        return v.x

    def gauss_seidel_(self, o, x, b, sweeps, direction="forward"):
        """`sweeps` exact Gauss-Seidel sweeps in place on x."""
        wave = smoothing.wavefront_gs(o, self.A, direction)
        smoothing.gauss_seidel(o, self.A, types.SimpleNamespace(x=x, b=b), wave, lambda: self.schedule(o, direction),
                               int(sweeps), direction)
        if wave:
            o.stencil_gs_check(self.A)   # one 4-byte read: a timed-out band must not return a wrong iterate silently

    def schedule(self, o, direction):
        if direction not in self.gs:
            A = self.A
            if direction == "backward":
                self.gs[direction] = self.schedule(o, "forward").reversed()
                smoothing.ask(o, "gs_prepare", A, self.gs[direction])
            else:
                self.gs[direction] = smoothing.gs_schedule(o, A, A.rowptr.cpu().numpy(), A.colidx.cpu().numpy(),
                                                           "lexicographic", A.device)
        return self.gs[direction]


_handles = {}        # int -> Operator
_library = None      # the torch.library.Library, kept alive


def _csr(rowptr, colidx, vals, ncols):
    return DeviceCSR(rowptr, colidx, vals, (rowptr.numel() - 1, ncols))


def _get(h):
    if h not in _handles:
        raise LmgError("unknown operator handle %d" % h)
    return _handles[h]


def _residual(A, x, b, r):
    part = torch.empty(ops.partials_count(A.shape[0]), dtype=F64, device=x.device)
    n2 = torch.empty(1, dtype=F64, device=x.device)
    ops.csr_residual_norm2(A, x, b, r, part, n2)
    return r, n2


def _gershgorin(o, A):
    out = torch.empty(1, dtype=F64, device=A.vals.device)
    o.csr_gershgorin(A, out)
    return out


def _jacobi(rowptr, colidx, vals, x, b, omega):
    out = torch.empty_like(x)
    ops.csr_jacobi(_csr(rowptr, colidx, vals, x.numel()), x, b, omega, out)
    return out


def _spmv(A, x):
    y = torch.empty(A.shape[0], dtype=F64, device=x.device)
    ops.csr_spmv(A, x, y, 1.0, 0.0)
    return y


def _line_factor(rowptr, colidx, vals, line_stride, dir):
    (lo, minv, cp), flags = ops.line_factor_flags(_csr(rowptr, colidx, vals, rowptr.numel() - 1), line_stride, dir)
    return lo, minv, cp, flags


def _line_factor_banded(rowptr, colidx, vals, line_stride, dir, band):
    return ops.line_factor_banded_flags(_csr(rowptr, colidx, vals, rowptr.numel() - 1), line_stride, dir, band)


def _spgemm(arp, aci, ava, acols, brp, bci, bva, bcols):
    C = ops.spgemm(_csr(arp, aci, ava, acols), _csr(brp, bci, bva, bcols))
    return C.rowptr, C.colidx, C.vals


def _transpose(rowptr, colidx, vals, ncols):
    T = _csr(rowptr, colidx, vals, ncols).transpose()
    return T.rowptr, T.colidx, T.vals


def _dense_gemv(M, x):
    y = torch.empty(M.shape[0], dtype=F64, device=x.device)
    ops.dense_gemv(M.contiguous(), x, y)
    return y


def _multi_dot(V, k, w):
    part = torch.empty(ops.multi_partials_count(w.numel(), k), dtype=F64, device=w.device)
    out = torch.zeros(int(k), dtype=F64, device=w.device)
    ops.multi_dot(V, k, w, part, out)
    return out


def _multi_axpy_(V, k, coef, w, subtract):
    part = torch.empty(ops.multi_partials_count(w.numel(), k), dtype=F64, device=w.device)
    n2 = torch.zeros(1, dtype=F64, device=w.device)
    ops.multi_axpy(V, k, coef, w, part, n2, subtract=bool(subtract))
    return n2


def _create(rowptr, colidx, vals, ncols):
    A = _csr(rowptr, colidx, vals, ncols)
    A.pack()
    h = 1 + max(_handles, default=0)
    _handles[h] = Operator(A)
    return h


def _format(h):
    A = _get(h).A
    return ("stencil" if A.stencil is not None else "rpat" if A.patterns is not None else
            "sell" if A.sell is not None else "pcsr" if A.packed is not None else "csr")


def _free(h):
    _handles.pop(h, None)


CUDA, ANY = "CUDA", "CompositeExplicitAutograd"
# (schema, implementation, dispatch key) of every op
OPS = [
    ("csr_residual(Tensor rowptr, Tensor colidx, Tensor vals, Tensor x, Tensor b) -> (Tensor, Tensor)",
     lambda rowptr, colidx, vals, x, b: _residual(_csr(rowptr, colidx, vals, x.numel()), x, b, torch.empty_like(x)), CUDA),
    ("csr_jacobi(Tensor rowptr, Tensor colidx, Tensor vals, Tensor x, Tensor b, float omega) -> Tensor", _jacobi, CUDA),
    ("csr_spmv(Tensor rowptr, Tensor colidx, Tensor vals, int ncols, Tensor x) -> Tensor",
     lambda rowptr, colidx, vals, ncols, x: _spmv(_csr(rowptr, colidx, vals, ncols), x), CUDA),
    ("csr_gs_rows_(Tensor rowptr, Tensor colidx, Tensor vals, Tensor(a!) x, Tensor b, Tensor rows) -> ()",
     lambda rowptr, colidx, vals, x, b, rows: ops.csr_gs_rows(_csr(rowptr, colidx, vals, x.numel()), x, b, rows), CUDA),
    # the rest of the C ABI: Galerkin SpGEMM, coarse GEMV, and operators with their lossless twins
    ("spgemm(Tensor a_rowptr, Tensor a_colidx, Tensor a_vals, int a_cols, Tensor b_rowptr, Tensor b_colidx, "
     "Tensor b_vals, int b_cols) -> (Tensor, Tensor, Tensor)", _spgemm, CUDA),
    ("csr_transpose(Tensor rowptr, Tensor colidx, Tensor vals, int ncols) -> (Tensor, Tensor, Tensor)", _transpose, CUDA),
    ("dense_gemv(Tensor M, Tensor x) -> Tensor", _dense_gemv, CUDA),
    # an operator handle owns the packed / row-pattern / stencil / sliced-ELL twin built once by pack()
    ("operator_create(Tensor rowptr, Tensor colidx, Tensor vals, int ncols) -> int", _create, CUDA),
    ("operator_format(int handle) -> str", _format, ANY),
    ("operator_free(int handle) -> ()", _free, ANY),
    ("operator_spmv(int handle, Tensor x) -> Tensor", lambda h, x: _spmv(_get(h).A, x), CUDA),
    ("operator_residual(int handle, Tensor x, Tensor b) -> (Tensor, Tensor)",
     lambda h, x, b: _residual(_get(h).A, x, b, torch.empty_like(b)), CUDA),
    ("operator_jacobi(int handle, Tensor x, Tensor b, float omega, int sweeps) -> Tensor",
     lambda h, x, b, omega, sweeps: _get(h).jacobi(ops, x, b, omega, sweeps), CUDA),
    ("operator_chebyshev(int handle, Tensor x, Tensor b, int degree, float lmax, float ratio) -> Tensor",
     lambda h, x, b, degree, lmax, ratio: _get(h).chebyshev(ops, x, b, degree, lmax, ratio), CUDA),
    ("operator_gershgorin(int handle) -> Tensor", lambda h: _gershgorin(ops, _get(h).A), ANY),
    ("cheby_update_(float a, float c, bool first, Tensor dinv, Tensor r, Tensor(a!) d, Tensor(b!) x) -> ()",
     lambda a, c, first, dinv, r, d, x: ops.cheby_update(a, c, dinv, r, d, x, first), CUDA),
    ("csr_gershgorin(Tensor rowptr, Tensor colidx, Tensor vals) -> Tensor",
     lambda rowptr, colidx, vals: _gershgorin(ops, _csr(rowptr, colidx, vals, rowptr.numel() - 1)), CUDA),
    ("operator_gauss_seidel_(int handle, Tensor(a!) x, Tensor b, int sweeps) -> ()",
     lambda h, x, b, sweeps: _get(h).gauss_seidel_(ops, x, b, sweeps), CUDA),
    ("operator_gauss_seidel_backward_(int handle, Tensor(a!) x, Tensor b, int sweeps) -> ()",
     lambda h, x, b, sweeps: _get(h).gauss_seidel_(ops, x, b, sweeps, "backward"), CUDA),
    ("line_factor(Tensor rowptr, Tensor colidx, Tensor vals, int line_stride, str dir) -> (Tensor, Tensor, Tensor, int)",
     _line_factor, CUDA),
    ("line_solve(int line_stride, str dir, int first, int step, Tensor lo, Tensor minv, Tensor cp, Tensor(a!) r, "
     "float omega, Tensor(b!) x) -> ()",
     lambda line_stride, dir, first, step, lo, minv, cp, r, omega, x:
         ops.line_solve(line_stride, dir, first, step, (lo, minv, cp), r, omega, x), CUDA),
    ("line_factor_banded(Tensor rowptr, Tensor colidx, Tensor vals, int line_stride, str dir, int band) -> (Tensor, int)",
     _line_factor_banded, CUDA),
    ("line_solve_banded(int line_stride, str dir, int band, int first, int step, Tensor fac, Tensor(a!) r, float omega, "
     "Tensor(b!) x) -> ()",
     lambda line_stride, dir, band, first, step, fac, r, omega, x:
         ops.line_solve_banded(line_stride, dir, band, first, step, fac, r, omega, x), CUDA),
    # the fused Gram-Schmidt passes of the Krylov solvers: V is a 2-D contiguous basis, k its rows in use
    ("multi_dot(Tensor V, int k, Tensor w) -> Tensor", _multi_dot, CUDA),
    ("multi_axpy_(Tensor V, int k, Tensor coef, Tensor(a!) w, bool subtract) -> Tensor", _multi_axpy_, CUDA),
]


def register():
    """Define and implement every op of the "lmg" library (once per process)."""
    global _library
    if _library is None:
        _library = torch.library.Library("lmg", "DEF")
        for schema, fn, key in OPS:
            _library.define(schema)
            _library.impl(schema[:schema.index("(")], fn, key)
