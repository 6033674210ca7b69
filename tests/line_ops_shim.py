"""TEST-ONLY: tests/cpu_ops_shim.py plus the ops of the line relaxation smoother, implemented by its CPU twin
(tests/line_ref.py).  base() returns a fresh namespace; every line_factor / line_solve / residual / copy call is recorded in
ns.calls so that a test can read the launch sequence of a cycle."""
import types

import numpy as np
import scipy.sparse as sp
import torch

import cpu_ops_shim as shim
import line_ref as LR


def _np(t):
    return t.numpy()


def _sp(A):
    return sp.csr_matrix((_np(A.vals), _np(A.colidx), _np(A.rowptr)), shape=A.shape)


def base():
    ns = types.SimpleNamespace(**{k: getattr(shim, k) for k in dir(shim) if not k.startswith("__")})
    ns.calls = []

    def line_factor(A, W, dir):
        fac, flags = LR.factor(_sp(A), int(W), dir)
        ns.calls.append(("factor", A.shape[0], int(W), dir))
        if flags & LR.COUPLED:
            raise ValueError("a non-zero entry couples two x-lines (an entry across the end of a line)")
        if flags & LR.PIVOT:
            raise ValueError("a zero or non-finite pivot in the %s-line systems" % dir)
        return tuple(torch.from_numpy(v) for v in fac)

    def line_solve(W, dir, first, step, fac, r, omega, x):
        xn, rn = LR.solve(tuple(_np(v) for v in fac), int(W), dir, int(first), int(step), _np(r), float(omega), _np(x))
        _np(x)[:] = xn
        _np(r)[:] = rn
        ns.calls.append(("solve", x.numel(), dir, int(first), int(step), float(omega)))

    def csr_residual_norm2(A, x, b, r, partials, norm2):
        shim.csr_residual_norm2(A, x, b, r, partials, norm2)
        ns.calls.append(("residual", A.shape[0]))

    def copy(src, dst):
        shim.copy(src, dst)
        ns.calls.append(("copy", src.numel()))

    ns.line_factor, ns.line_solve, ns.csr_residual_norm2, ns.copy = line_factor, line_solve, csr_residual_norm2, copy
    return ns
