"""The multigrid preconditioner of the Krylov solvers (CG, GMRES): one cycle of a Hierarchy from a zero guess per application,
the smoother check that goes with it, and what the solve_many methods share (hierarchy_stream, check_columns, BlockSolves)."""
import contextlib

import numpy as np
import torch

from .. import ops
from ..smoothing import gs_mode_name, smoother_options

SMOOTHERS = ("Jacobi", "GaussSeidel", "Chebyshev", "Line")


@contextlib.contextmanager
def hierarchy_stream(H, device):
    """The body runs on the hierarchy's stream (a cycle is captured there), behind what the current stream holds, and the
    current stream waits for it afterwards.  H None: the current stream."""
    side = None if H is None else H.stream
    if side is not None:
        side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):                                  # (None: the current stream)
        yield
    if side is not None:
        torch.cuda.current_stream(device).wait_stream(side)


def check_columns(rhs, initial_guess, n):
    """(B, X0) of a solve_many: rhs as an (n, m) fp64 array, m >= 1, and initial_guess in its shape or None (ValueError)."""
    B = np.asarray(rhs, dtype=np.float64)
    if B.ndim != 2 or B.shape[0] != n or B.shape[1] < 1:
        raise ValueError("rhs must be (n, m) with n = %d and m >= 1, got %s" % (n, B.shape))
    X0 = None
    if initial_guess is not None:
        X0 = np.asarray(initial_guess, dtype=np.float64)
        if X0.shape != B.shape:
            raise ValueError("initial_guess must have the shape of rhs %s, got %s" % (B.shape, X0.shape))
    return B, X0


class BlockSolves:
    """What the solve_many methods share (a mixin in front of IterativeSolver): one BlockCycle per width of the hierarchy in
    use, kept from call to call (_block_cycle), and for CG and GMRES the operator's fp64 sliced-ELL twin, the checks of rhs
    and initial_guess and the streams (_solve_many; a solver that does not call it, Multigrid, never builds the twin)."""

    def _reset_blocks(self):
        self._block_cycles = {}            # {"H": the hierarchy, k: its BlockCycle of width k}
        self._block_twin = None            # the operator's fp64 sliced-ELL twin

    def _invalidate(self):
        super()._invalidate()
        self._reset_blocks()

    def _block_cycle(self, H, mc):
        """The cached BlockCycle of the hierarchy H for a chunk of mc columns, ready for them (use_columns)."""
        from ..block import BlockCycle, block_width
        if self._block_cycles.get("H") is not H:                   # (one hierarchy at a time: a new one drops the old blocks)
            self._block_cycles = {"H": H}
        k = block_width(mc, ops.BLOCK_WIDTHS)
        bc = self._block_cycles.get(k)
        if bc is None:
            bc = self._block_cycles[k] = BlockCycle(H, mc)
        bc.use_columns(mc)
        return bc

    def _solve_many(self, rhs, initial_guess, H, columns):
        """columns(A, block_cycle, B, X0, device) -> (X, track, iterations) on the hierarchy's stream: A the block twin,
        block_cycle(mc) H's BlockCycle for a chunk of mc columns (None without H).  Sets iterations_many, returns (X, track)."""
        B, X0 = check_columns(rhs, initial_guess, self.dim)
        dev = self._device
        A = self._device_matrix()
        A.pack()
        if self._block_twin is None:
            self._block_twin = ops.block_twin(A)
        with hierarchy_stream(H, dev):
            X, track, its = columns(self._block_twin, lambda mc: None if H is None else self._block_cycle(H, mc), B, X0, dev)
        self.iterations_many = its
        return X, track


def check_smoother(smoother, steps, **keywords):
    """What CG.solve and GMRES.solve check before any device work: the smoother name, and its `steps` and keywords by
    smoothing.smoother_options.  Returns the options make_apply prepares the hierarchy with."""
    if smoother not in SMOOTHERS:
        raise ValueError("precond_smoother must be 'Jacobi', 'GaussSeidel', 'Chebyshev' or 'Line', got %r" % (smoother,))
    return smoother_options(smoother, steps, **keywords)


def gs_mode_keyword(precond_gs_mode):
    """The precond_gs_mode of CG.solve and GMRES.solve as the keyword of make_apply, checked (ValueError): {} for the default
    ordering, which make_apply is not told -- it was called with seven arguments before it had the keyword, and still is."""
    gs_mode_name(precond_gs_mode, "precond_gs_mode")
    return {} if precond_gs_mode == "lexicographic" else {"gs_mode": precond_gs_mode}


def make_apply(H, smoother, steps, omega, shape, gs_sweep, options, gs_mode="lexicographic", k_inner=None):
    """apply_M(src, dst): dst = one `shape` cycle of H on the right-hand side src from a zero guess (H None: dst = src).
    Prepares what the smoother needs on the hierarchy (options, from check_smoother: Chebyshev bounds and work vectors, line
    factors) before the first application; a smoother without options sets itself up in its first sweep.  gs_sweep: the
    (pre, post) directions of a Gauss-Seidel cycle and gs_mode its ordering (smoothing.GS_MODES); a smoother with no use for
    them, or for omega, hands them to no launch.  k_inner: the inner method of a "K" cycle (None: Hierarchy.cycle's default)."""
    if H is not None and options:
        H.prepare_smoother(smoother, **options)
    krylov_kw = {} if k_inner is None else {"k_inner": k_inner}

    def apply_M(src, dst):
        if H is None:
            ops.copy(src, dst)
            return
        fine = H.levels[0]
        ops.copy(src, fine.b)
        H.cycle(smoother, steps, omega, gs_mode, x_is_zero=True, gs_sweep=gs_sweep, shape=shape, **krylov_kw)
        ops.copy(fine.x, dst)

    return apply_M
