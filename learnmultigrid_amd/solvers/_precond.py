"""The multigrid preconditioner of the Krylov solvers (CG, GMRES): one cycle of a Hierarchy from a zero guess per
application, the smoother-name check that goes with it, and what their solve_many methods share (BlockSolves)."""
import numpy as np
import torch

from .. import ops
from ..hierarchy import line_band_value, line_config

SMOOTHERS = ("Jacobi", "GaussSeidel", "Chebyshev", "Line")


class BlockSolves:
    """What CG.solve_many and GMRES.solve_many share (a mixin in front of IterativeSolver): the operator's fp64 sliced-ELL
    twin and one BlockCycle per width, kept from call to call, the checks of rhs and initial_guess, and the streams."""

    def _reset_blocks(self):
        self._block_cycles = {}            # {"H": the preconditioner, k: its BlockCycle of width k}
        self._block_twin = None            # the operator's fp64 sliced-ELL twin

    def _invalidate(self):
        super()._invalidate()
        self._reset_blocks()

    def _solve_many(self, rhs, initial_guess, H, columns):
        """columns(A, block_cycle, B, X0, device) -> (X, track, iterations) on the hierarchy's stream (a cycle is captured
        there; the current stream without a preconditioner): A the block twin, block_cycle(mc) the cached BlockCycle of H
        for a chunk of mc columns, ready for them, or None.  Sets iterations_many and returns (X, track)."""
        B = np.asarray(rhs, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != self.dim or B.shape[1] < 1:
            raise ValueError("rhs must be (n, m) with n = %d and m >= 1, got %s" % (self.dim, B.shape))
        X0 = None
        if initial_guess is not None:
            X0 = np.asarray(initial_guess, dtype=np.float64)
            if X0.shape != B.shape:
                raise ValueError("initial_guess must have the shape of rhs %s, got %s" % (B.shape, X0.shape))
        from ..block import BlockCycle, block_width
        dev = self._device
        A = self._device_matrix()
        A.pack()
        if self._block_twin is None:
            self._block_twin = ops.block_twin(A)
        if self._block_cycles.get("H") is not H:                   # (one hierarchy at a time: a new one drops the old blocks)
            self._block_cycles = {"H": H}

        def block_cycle(mc):
            if H is None:
                return None
            k = block_width(mc, ops.BLOCK_WIDTHS)
            bc = self._block_cycles.get(k)
            if bc is None:
                bc = self._block_cycles[k] = BlockCycle(H, mc)
            bc.use_columns(mc)
            return bc

        side = None if H is None else H.stream
        if side is not None:
            side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                              # (None: the current stream)
            X, track, its = columns(self._block_twin, block_cycle, B, X0, dev)
        if side is not None:
            torch.cuda.current_stream(dev).wait_stream(side)
        self.iterations_many = its
        return X, track


def check_smoother(smoother, line_dir, line_order, line_band=None):
    """The smoother name and, for "Line", its keywords: what CG.solve and GMRES.solve check before any device work."""
    if smoother not in SMOOTHERS:
        raise ValueError("precond_smoother must be 'Jacobi', 'GaussSeidel', 'Chebyshev' or 'Line', got %r" % (smoother,))
    if smoother == "Line":
        line_config(line_dir, line_order)
        line_band_value(line_band)


def prepare_line_band(H, smoother, line_dir, line_order, line_band):
    """For the "Line" smoother: factor H's levels with the largest half-bandwidth line_band (None = 1) before make_apply,
    which then keeps the band in use."""
    if H is not None and smoother == "Line":
        H.prepare_smoother("Line", line_dir=line_dir, line_order=line_order, line_band=1 if line_band is None else line_band)


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
