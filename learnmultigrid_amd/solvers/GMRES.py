"""Restarted flexible GMRES -- the Krylov solver for what CG cannot take: operators that are not symmetric (the grid
problems of problems.py keep their Dirichlet rows as identity rows and leave the columns alone) and preconditioners that
are not symmetric operators (forward Gauss-Seidel on both sides of the coarse correction, the cycle the reference ships;
F-cycles).  The reference has no such class; the conventions are those of CG: the initial residual is track_res[0], one
entry per iteration after it, stop on ||r|| <= error.

`preconditioner=Hierarchy` preconditions from the right with one cycle from a zero guess per iteration, with CG's
keywords; `precond_cycle_shape` also takes "F" and "K" (the Krylov-accelerated cycle with `precond_k_inner` = "gcr" | "fcg": a
nonlinear preconditioner, which a flexible method may take), and `precond_gs_sweep` any sweep name or (pre, post) pair of
Hierarchy.cycle (default forward / forward); `precond_line_band` and `precond_gs_mode` as in CG.solve.  The iteration is krylov.fgmres: classical Gram-Schmidt applied twice in four
fused launches and one device-to-host read per iteration; its residual estimate is the true residual norm in exact
arithmetic, and the true norm is recomputed at the end of every cycle of `restart` iterations.  Memory: 2 restart + 1
vectors for the bases, (2 restart + 4) 8 n bytes with x, b and the scratch.

`solve_many(rhs, ...)` solves for the columns of an (n, m) matrix of right-hand sides on blocks of 2, 4 or 8 interleaved
columns (krylov.block_fgmres): every column runs the same recurrence on its own numbers, the block shares the matrix bytes of
the cycle and of A z, the launches and the host read."""
import numpy as np
import torch

from .. import krylov, ops
from ..hierarchy import KRYLOV_SHAPES, cycle_children, gs_sweep_pair, k_inner_name, linear_cycle_children
from ..ops import F64
from ._precond import BlockSolves, check_smoother, gs_mode_keyword, make_apply
from .Solver import IterativeSolver, on_device


def check_keywords(restart, max_vectors, precond_smoother, precond_cycle_shape, precond_gs_sweep, precond_line_dir,
                   precond_line_order, precond_line_band=None, precond_steps=2):
    """The keyword checks of GMRES.solve (ValueError); returns (pair, options): the (pre, post) Gauss-Seidel directions and
    the smoother options make_apply prepares the hierarchy with (check_smoother).  max_vectors: the most basis rows a
    Gram-Schmidt launch takes (ops.krylov_max_vectors()): a cycle holds restart + 1."""
    check_restart(restart, max_vectors)
    options = check_smoother(precond_smoother, precond_steps, line_dir=precond_line_dir, line_order=precond_line_order,
                             line_band=precond_line_band)
    cycle_children(precond_cycle_shape)
    return gs_sweep_pair(precond_gs_sweep), options


def check_restart(restart, max_vectors):
    """restart is an integer in 1 .. max_vectors - 1 (ValueError): a cycle's basis holds restart + 1 vectors, and
    max_vectors (ops.krylov_max_vectors()) is the most a Gram-Schmidt launch takes."""
    if int(restart) != restart or restart < 1:
        raise ValueError("restart must be an integer >= 1, got %r" % (restart,))
    if restart >= max_vectors:
        raise ValueError("restart must be < %d (the Gram-Schmidt kernels take %d basis vectors), got %r"
                         % (max_vectors, max_vectors, restart))


class GMRES(BlockSolves, IterativeSolver):

    def __init__(self, matrix, rhs, **kw):
        super().__init__(matrix, rhs, **kw)
        self._log("Selected GMRES")
        self.label = "GMRES"
        self._reset_blocks()               # solve_many's caches

    @on_device
    def solve(self, max_iterations=1000, error=1e-08, initial_guess=None, *, restart=30, preconditioner=None,
              precond_steps=2, precond_omega=0.8, precond_smoother="Jacobi", precond_cycle_shape="V",
              precond_gs_sweep="forward", precond_line_dir="xy", precond_line_order="zebra",
              precond_line_band=None, precond_gs_mode="lexicographic", precond_k_inner="gcr"):
        gs_mode_keyword(precond_gs_mode)
        k_inner_name(precond_k_inner)
        pair, options = check_keywords(restart, ops.krylov_max_vectors(), precond_smoother, precond_cycle_shape, precond_gs_sweep,
                                       precond_line_dir, precond_line_order, precond_line_band, precond_steps)
        A = self._device_matrix()
        A.pack()
        n = self.dim
        dev = self._device
        b = self._to_device(self.rhs)
        x = torch.zeros(n, dtype=F64, device=dev) if initial_guess is None else self._to_device(initial_guess)
        r = torch.empty_like(x)
        H = preconditioner
        apply_M = None
        if H is not None:
            krylov_kw = {"k_inner": precond_k_inner} if precond_cycle_shape in KRYLOV_SHAPES else {}
            apply_M = make_apply(H, precond_smoother, precond_steps, precond_omega, precond_cycle_shape, pair, options,
                                 **gs_mode_keyword(precond_gs_mode), **krylov_kw)
        track, self.iterations = krylov.fgmres(ops, A, b, x, apply_M, restart=int(restart), max_iterations=max_iterations,
                                               error=error, residual_out=r)
        if track[-1] <= error:
            self._log("Reached convergence")
        if H is not None and precond_smoother == "GaussSeidel":
            H.check_smoothers()            # a timed-out wavefront band raises instead of leaving a wrong solution
        self.residual = track[-1]
        self.solution = self._column(x)
        self.residual_vector = self._column(r)
        self.track_res = np.array(track, dtype=float).reshape(-1, 1)

    # -- several right-hand sides at once (no counterpart in the reference) ----------------------
    @on_device
    def solve_many(self, rhs, max_iterations=1000, error=1e-08, initial_guess=None, *, restart=30, preconditioner=None,
                   precond_steps=2, precond_omega=0.8, precond_cycle_shape="V", use_graph=False):
        """Solve A X = rhs for the m >= 1 columns of rhs (n, m) by restarted flexible GMRES on blocks of columns
        (krylov.block_fgmres): the operator and, with preconditioner=Hierarchy, every matrix of the hierarchy are read once
        per iteration for up to 8 columns, the Gram-Schmidt passes of the columns share four launches, and one
        device-to-host read per iteration serves them all.  Every column runs the recurrence of solve() on its own numbers
        and stops on its own: at its estimate within a cycle, for good once its recomputed true norm is <= error or it has
        run max_iterations inner iterations; its X is not stored after that, while the other columns of its chunk go on.
        Columns are padded with zero columns to a width of 2, 4 or 8 and worked through in chunks of 8, like
        Multigrid.solve_many.  Returns (X, track): X (n, m); column j of track is what solve() records for that column, in
        the column's OWN iteration count -- row 0 the true ||b_j - A x_j||_2 of the initial guess, row i its i-th inner
        iteration (the Arnoldi estimate; the recomputed true norm for the last iteration of each of its cycles) --, NaN
        behind its last iteration.  self.iterations_many[j]: the inner iterations column j ran (0: it started at or below
        error).
        The preconditioner is one precond_cycle_shape ("V" | "W" | "F"; "K" raises ValueError) cycle of block.BlockCycle from
        a zero guess per iteration, which smooths with weighted Jacobi only (precond_steps sweeps before and after, damping precond_omega):
        no other smoother can be asked for here.  A hierarchy with cycle_values="f32" is refused by BlockCycle.  use_graph
        replays the cycle from a captured hipGraph; everything else of an iteration is launched as it is.  solve() is not
        touched by any of this."""
        check_restart(restart, ops.krylov_max_vectors())
        linear_cycle_children(precond_cycle_shape, "GMRES.solve_many")

        def columns(A, block_cycle, B, X0, dev):
            return krylov.block_fgmres_columns(ops, A, block_cycle, B, X0, dev, restart=int(restart),
                                               max_iterations=int(max_iterations), error=error, steps=precond_steps,
                                               omega=precond_omega, shape=precond_cycle_shape, use_graph=bool(use_graph))

        return self._solve_many(rhs, initial_guess, preconditioner, columns)
