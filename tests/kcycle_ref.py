"""CPU restatement of the K-cycle -- TEST INFRASTRUCTURE ONLY.

What the K-cycle tests share:

  * the recurrence of the two inner Krylov steps in NumPy (step1_coefficients / step2_coefficients and the two vector lines),
    every product and sum on a line of its own, which is what the kernels round like;
  * kcycle_step1 / kcycle_step2, stand-ins of the ops of those names on CPU tensors, handed to a Hierarchy through
    cpu_ops_shim.namespace(kcycle_step1=..., kcycle_step2=...) (ops_namespace() does that);
  * KCycle, the twin of Hierarchy.cycle(shape="K"): cycle_shapes_ref.ShapeCycle whose coarse visits are two steps of flexible
    GCR or CG from a zero iterate, preconditioned by the K-cycle visit of the level;
  * aggregation_hierarchy, plain 3 x 3 aggregation of an s x s grid with a piecewise-constant P: the kind of hierarchy whose
    V-cycle degrades with the number of levels.
"""
import numpy as np
import scipy.sparse as sp

import cpu_ops_shim as shim
from cycle_shapes_ref import ShapeCycle
from oracle import kernels as K
from support import to_numpy as _np

K_INNER = ("gcr", "fcg")
SCALARS = ("alpha1", "rho1", "t1", "gamma", "beta", "alpha2", "rho2", "t2", "a")      # the layout of `scal`


def step1_coefficients(alpha1, rho1):
    """t1 from the two products of step 1."""
    alpha1, rho1 = np.float64(alpha1), np.float64(rho1)
    with np.errstate(all="ignore"):
        return alpha1 / rho1 if rho1 != 0.0 else np.float64(0.0)


def step1_vector(b, v1, t1):
    """rt = b + (-t1) * v1, the product rounded before the sum."""
    return b + (-np.float64(t1)) * v1


def step2_coefficients(rho1, t1, gamma, beta, alpha2):
    """(rho2, t2, a) from the three products of step 2 and what step 1 left."""
    rho1, t1, gamma, beta, alpha2 = (np.float64(v) for v in (rho1, t1, gamma, beta, alpha2))
    with np.errstate(all="ignore"):
        q = gamma / rho1 if rho1 != 0.0 else np.float64(0.0)
        gq = gamma * q
        rho2 = beta - gq
        t2 = alpha2 / rho2 if rho2 != 0.0 else np.float64(0.0)
        qt = q * t2
        a = t1 - qt
    return rho2, t2, a


def step2_vector(c1, c2, a, t2):
    """x = a * c1 + t2 * c2, both products rounded before the sum."""
    return np.float64(a) * c1 + np.float64(t2) * c2


def direction(k_inner, c, v):
    if k_inner not in K_INNER:
        raise ValueError(k_inner)
    return v if k_inner == "gcr" else c


def two_steps(k_inner, visit, matvec, b):
    """x_c of an accelerated visit: visit(rhs) -> the level's cycle from zero, matvec(x) -> A x."""
    c1 = visit(b)
    v1 = matvec(c1)
    p1 = direction(k_inner, c1, v1)
    alpha1, rho1 = float(np.dot(p1, b)), float(np.dot(p1, v1))
    t1 = step1_coefficients(alpha1, rho1)
    rt = step1_vector(b, v1, t1)
    c2 = visit(rt)
    v2 = matvec(c2)
    p2 = direction(k_inner, c2, v2)
    gamma, beta, alpha2 = float(np.dot(p2, v1)), float(np.dot(p2, v2)), float(np.dot(p2, rt))
    _rho2, t2, a = step2_coefficients(rho1, t1, gamma, beta, alpha2)
    return step2_vector(c1, c2, a, t2)


# ---- stand-ins of ops.kcycle_step1 / ops.kcycle_step2 on CPU tensors ------------------------------------------------------
def kcycle_step1(k_inner, c1, v1, b, rt, scal, partials, form="auto"):
    c, v, bb = _np(c1), _np(v1), _np(b)
    p = direction(k_inner, c, v)
    alpha1, rho1 = float(np.dot(p, bb)), float(np.dot(p, v))
    t1 = step1_coefficients(alpha1, rho1)
    _np(rt)[:] = step1_vector(bb, v, t1)
    _np(scal)[0:3] = (alpha1, rho1, t1)


def kcycle_step2(k_inner, c1, v1, c2, v2, rt, scal, x_out, partials, form="auto"):
    ca, va, cb, vb, r, s = _np(c1), _np(v1), _np(c2), _np(v2), _np(rt), _np(scal)
    p = direction(k_inner, cb, vb)
    gamma, beta, alpha2 = float(np.dot(p, va)), float(np.dot(p, vb)), float(np.dot(p, r))
    rho2, t2, a = step2_coefficients(s[1], s[2], gamma, beta, alpha2)
    _np(x_out)[:] = step2_vector(ca, cb, a, t2)               # (the right side is complete before x_out, maybe c2, is written)
    s[3:9] = (gamma, beta, alpha2, rho2, t2, a)


def ops_namespace(**replace):
    """The CPU stand-in of ops with the two K-cycle ops: what Hierarchy(ops_mod=...) runs K-cycles on."""
    return shim.namespace(**{"kcycle_step1": kcycle_step1, "kcycle_step2": kcycle_step2, **replace})


# ---- the twin -------------------------------------------------------------------------------------------------------------
class KCycle(ShapeCycle):

    def __init__(self, A, hierarchy, k_inner="gcr", gs_sweep=("forward", "forward")):
        super().__init__(A, hierarchy, "K", gs_sweep)
        direction(k_inner, None, None)
        self.k_inner = k_inner

    def cycle(self, x, b, smoother="Jacobi", steps=3, omega=1.0, l=0, shape=None):
        b = np.ascontiguousarray(b, dtype=float).reshape(-1)
        x = self.smooth_dir(l, np.ascontiguousarray(x, dtype=float).reshape(-1).copy(), b, smoother, steps, omega,
                            self.gs_sweep[0])
        r, _ = K.residual(self.A[l], x, b)
        rc = K.matvec(self.R[l], r)
        if l + 1 == len(self.P):
            ec = self.lu.solve(rc)
        else:
            ec = two_steps(self.k_inner, lambda rhs: self.cycle(np.zeros_like(rhs), rhs, smoother, steps, omega, l + 1),
                           lambda v: K.matvec(self.A[l + 1], v), rc)
        x = K.spmv(self.P[l], ec, x, 1.0, 1.0)
        return self.smooth_dir(l, x, b, smoother, steps, omega, self.gs_sweep[1])


# ---- plain aggregation ----------------------------------------------------------------------------------------------------
def aggregation_hierarchy(side, levels):
    """levels - 1 transfers of an s x s grid in row-major order, s = side, ceil(s / 3), ...: node (i, j) belongs to aggregate
    (i // 3, j // 3) and P has an entry of 1 there."""
    out = []
    s = int(side)
    for _ in range(levels - 1):
        sc = (s + 2) // 3
        i, j = np.divmod(np.arange(s * s), s)
        agg = (i // 3) * sc + (j // 3)
        out.append(sp.csr_matrix((np.ones(s * s), (np.arange(s * s), agg)), shape=(s * s, sc * sc)))
        s = sc
    return out
