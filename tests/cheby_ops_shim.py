"""TEST-ONLY: tests/cpu_ops_shim.py plus the ops of the Chebyshev smoother, implemented by its CPU twin
(tests/chebyshev_ref.py).  base(): the two-launch path only; fused(): also stand-ins of the tiled Chebyshev passes, each
computing what the separate launches would and recording the call."""
import types

import numpy as np
import scipy.sparse as sp

import chebyshev_ref as C
import cpu_ops_shim as shim
from oracle import kernels as K


def _np(t):
    return t.numpy()


def _sp(A):
    return sp.csr_matrix((_np(A.vals), _np(A.colidx), _np(A.rowptr)), shape=A.shape)


def cheby_update(a, c, dinv, r, d, x, first=False):
    z = _np(dinv) * _np(r)
    dn = c * z if first else a * _np(d) + c * z
    _np(d)[:] = dn
    _np(x)[:] = _np(x) + dn


def csr_gershgorin(A, out):
    _np(out)[0] = C.gershgorin(_sp(A))


def base():
    ns = types.SimpleNamespace(**{k: getattr(shim, k) for k in dir(shim) if not k.startswith("__")})
    ns.cheby_update = cheby_update
    ns.csr_gershgorin = csr_gershgorin
    ns.calls = []
    return ns


def fused(max_rows=None):
    """max_rows: levels with more rows have no fused pass (the mix of both paths in one cycle)."""
    ns = base()
    ns.FUSED_MAX_SWEEPS = 3
    ok = (lambda A: True) if max_rows is None else (lambda A: A.shape[0] <= max_rows)
    ns.stencil_cheby_available = ok
    ns.stencil_cheby_prolong_available = lambda A, P_: ok(A)
    ns.stencil_cheby_restrict_available = lambda A, R: ok(A)
    # the Jacobi predicates exist and say yes: the Chebyshev cycle must not pick them up
    ns.stencil_smooth_available = lambda A: True
    ns.stencil_smooth_turnaround_selected = lambda A, P_, R: True

    def turn(*a, **k):
        raise AssertionError("the Chebyshev cycle has no turnaround pass")

    ns.stencil_smooth_turnaround = turn

    def stencil_cheby(A, x_in, b, coef, x_out, r_out=None, prolong=None, restrict=None):
        assert 1 <= len(coef) <= 3 and (prolong is None or restrict is None)
        As = _sp(A)
        bb = _np(b)
        x = np.zeros(A.shape[0]) if x_in is None else _np(x_in).copy()
        if prolong is not None:
            x = K.spmv(_sp(prolong[0]), _np(prolong[1]), x, 1.0, 1.0)
        x = C.cheby_step(As, x, bb, coef)
        _np(x_out)[:] = x
        r, _ = K.residual(As, x, bb)
        if r_out is not None:
            _np(r_out)[:] = r
        if restrict is not None:
            _np(restrict[1])[:] = K.matvec(_sp(restrict[0]), r)
        ns.calls.append(("prolong" if prolong is not None else "restrict" if restrict is not None else "plain",
                         A.shape[0], len(coef), x_in is None))

    ns.stencil_cheby = stencil_cheby
    return ns
