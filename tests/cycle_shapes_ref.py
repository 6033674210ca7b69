"""CPU restatement of the W- and F-cycles -- TEST INFRASTRUCTURE ONLY.

oracle.vcycle_ref.HoistedVCycle with the cycle shapes of pyamg's multilevel_solver (Hierarchy.cycle's convention):
after the restriction on level l, a V-cycle runs one V-cycle on level l + 1, a W-cycle two W-cycles, an F-cycle an
F-cycle then a V-cycle, the second call starting from the first one's iterate with the same right-hand side; on the
second-coarsest level the coarsest one is solved once, whatever the shape.  Gauss-Seidel may run forward, backward or
symmetric on either side (the backward sweep is the oracle's sweep over rows n-1 .. 0).
"""
import numpy as np

from oracle import kernels as K
from oracle import vcycle_ref as V

CHILDREN = {"V": ("V",), "W": ("W", "W"), "F": ("F", "V")}


class ShapeCycle(V.HoistedVCycle):

    def __init__(self, A, hierarchy, shape="V", gs_sweep=("forward", "forward")):
        super().__init__(A, hierarchy)
        self.shape = shape
        self.gs_sweep = (gs_sweep, gs_sweep) if isinstance(gs_sweep, str) else tuple(gs_sweep)

    def _gs(self, l, x, b, steps, direction):
        A = self.A[l]
        back = np.arange(A.shape[0] - 1, -1, -1, dtype=np.int32)
        for _ in range(steps):
            if direction in ("forward", "symmetric"):
                K.gs_forward(A, x, b, 1)
            if direction in ("backward", "symmetric"):
                K.gs_rows(A, x, b, back)
        return x

    def smooth_dir(self, l, x, b, smoother, steps, omega, direction):
        if smoother == "GaussSeidel":
            return self._gs(l, x, b, steps, direction)
        return self.smooth(l, x, b, smoother, steps, omega)

    def cycle(self, x, b, smoother="Jacobi", steps=3, omega=1.0, l=0, shape=None):
        shape = self.shape if shape is None else shape
        b = np.ascontiguousarray(b, dtype=float).reshape(-1)
        x = self.smooth_dir(l, np.ascontiguousarray(x, dtype=float).reshape(-1).copy(), b, smoother, steps, omega,
                            self.gs_sweep[0])
        r, _ = K.residual(self.A[l], x, b)
        rc = K.matvec(self.R[l], r)
        if l + 1 == len(self.P):
            ec = self.lu.solve(rc)
        else:
            ec = np.zeros_like(rc)
            for sub in CHILDREN[shape]:
                ec = self.cycle(ec, rc, smoother, steps, omega, l + 1, sub)
        x = K.spmv(self.P[l], ec, x, 1.0, 1.0)
        return self.smooth_dir(l, x, b, smoother, steps, omega, self.gs_sweep[1])


def history(ref, A, rhs, cycles, **kw):
    """||b - A x|| before each of `cycles` cycles from a zero guess, and the final iterate."""
    b = np.asarray(rhs, dtype=float).ravel()
    x = np.zeros(A.shape[0])
    out = []
    for _ in range(cycles):
        out.append(np.linalg.norm(b - A @ x))
        x = ref.cycle(x, b, **kw)
    return np.array(out), x
