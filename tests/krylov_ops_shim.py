"""TEST-ONLY: tests/cpu_ops_shim.py plus the fused Gram-Schmidt ops of the Krylov solvers in NumPy, so that the host logic
of learnmultigrid_amd/krylov.py runs on CPU tensors."""
import types

import cpu_ops_shim as shim

MAX_VECTORS = 65


def _np(t):
    return t.numpy()


def krylov_max_vectors():
    return MAX_VECTORS


def multi_partials_count(n, k):
    return 1024 * max(int(k), 1)


def multi_dot(V, k, w, partials, out):
    n = w.numel()
    assert V.dim() == 2 and V.is_contiguous() and 0 <= k <= min(V.shape[0], MAX_VECTORS) and V.shape[1] >= n
    if k:
        _np(out)[:k] = _np(V)[:k, :n] @ _np(w)


def multi_axpy(V, k, coef, w, partials=None, norm2=None, subtract=True):
    n = w.numel()
    assert V.dim() == 2 and V.is_contiguous() and 0 <= k <= min(V.shape[0], MAX_VECTORS) and V.shape[1] >= n
    ww, c = _np(w), _np(coef).copy()            # (coef may be a view of the buffer norm2 lives in)
    for j in range(k):
        ww[:] = ww - c[j] * _np(V)[j, :n] if subtract else ww + c[j] * _np(V)[j, :n]
    if norm2 is not None:
        assert partials is not None
        _np(norm2)[0] = float(ww @ ww)


def base():
    ns = types.SimpleNamespace(**{k: getattr(shim, k) for k in dir(shim) if not k.startswith("__")})
    ns.krylov_max_vectors = krylov_max_vectors
    ns.multi_partials_count = multi_partials_count
    ns.multi_dot = multi_dot
    ns.multi_axpy = multi_axpy
    return ns
