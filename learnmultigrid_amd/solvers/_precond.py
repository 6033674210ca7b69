"""The multigrid preconditioner of the Krylov solvers (CG, GMRES): one cycle of a Hierarchy from a zero guess per
application, and the smoother-name check that goes with it."""
from .. import ops
from ..hierarchy import line_config

SMOOTHERS = ("Jacobi", "GaussSeidel", "Chebyshev", "Line")


def check_smoother(smoother, line_dir, line_order):
    """The smoother name and, for "Line", its keywords: what CG.solve and GMRES.solve check before any device work."""
    if smoother not in SMOOTHERS:
        raise ValueError("precond_smoother must be 'Jacobi', 'GaussSeidel', 'Chebyshev' or 'Line', got %r" % (smoother,))
    if smoother == "Line":
        line_config(line_dir, line_order)


def make_apply(H, smoother, steps, omega, shape, gs_sweep, line_dir, line_order):
    """apply_M(src, dst): dst = one `shape` cycle of H on the right-hand side src from a zero guess (H None: dst = src).
    Prepares what the smoother needs on the hierarchy (Chebyshev bounds and work vectors, line factors) before the first
    application.  gs_sweep: the (pre, post) directions of a Gauss-Seidel cycle; the other smoothers do not use it."""
    if H is not None and smoother == "Chebyshev":
        H.prepare_smoother("Chebyshev")        # bounds and work vectors before the first application
    if H is not None and smoother == "Line":
        H.prepare_smoother("Line", line_dir=line_dir, line_order=line_order)

    def apply_M(src, dst):
        if H is None:
            ops.copy(src, dst)
            return
        fine = H.levels[0]
        ops.copy(src, fine.b)
        if smoother == "GaussSeidel":
            H.cycle("GaussSeidel", steps, 1.0, x_is_zero=True, gs_sweep=gs_sweep, shape=shape)
        elif smoother == "Chebyshev":
            H.cycle("Chebyshev", steps, 1.0, x_is_zero=True, shape=shape)
        elif smoother == "Line":
            H.cycle("Line", steps, omega, x_is_zero=True, shape=shape)
        else:
            H.cycle("Jacobi", steps, omega, x_is_zero=True, shape=shape)
        ops.copy(fine.x, dst)

    return apply_M
