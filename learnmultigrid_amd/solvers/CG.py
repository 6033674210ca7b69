"""Conjugate gradients -- mirrors learn_multigrid/solvers/CG.py:12-50 (same signature, the
initial residual is track_res[0], one entry per iteration after it, stop on ||r|| <= error).
The reference's CG only runs under NumPy < 1.23 (`np.asscalar`, CG.py:30,:32,:47); the
arithmetic is the textbook recurrence and is executed here by the HIP kernels (SpMV, dot,
axpby), two 8-byte D2H reads per iteration for alpha and beta.

Build-only extension (keyword-only): `preconditioner=Hierarchy` turns it into multigrid-
preconditioned CG -- one V(nu,nu) Jacobi cycle from a zero guess per application (the
"step after the hot path" of SURVEY.md section 8 f4).  precond_smoother="GaussSeidel" smooths with
nu forward Gauss-Seidel sweeps before and nu backward sweeps after the coarse correction instead:
with R = P^T, Galerkin coarse operators and the direct coarse solve that cycle is a symmetric
operator, the standard MG-PCG setup (each half is one pipelined launch of the wavefront kernel).
precond_cycle_shape="W" applies one W-cycle instead (Hierarchy.cycle); it is as symmetric as the V-cycle.  An F-cycle
is not (its second visits are V-cycles: the F-cycle's adjoint would run them first) and is rejected.
precond_smoother="Chebyshev" smooths with one Chebyshev polynomial step of degree precond_steps on either side: a polynomial
in D^-1 A applied to D^-1 is a symmetric operator, so the cycle is one too -- as parallel as the Jacobi cycle, no damping
parameter (precond_omega is not used; bounds as prepared on the hierarchy, Hierarchy.prepare_smoother).
precond_smoother="Line" smooths with precond_steps line relaxation steps (precond_line_dir "x" | "y" | "xy",
precond_line_order "zebra" | "jacobi", damping precond_omega: pass 1.0 for zebra) on either side; the post-smoothing half
runs the directions and colours in reverse, the adjoint of the pre-smoothing half, so the cycle is a symmetric operator --
the preconditioner for operators with a strong direction.  precond_line_band (1 | 2 | 3, None = 1) is the largest
half-bandwidth of the line systems (Hierarchy.prepare_smoother): 3 for the 25- and 49-point levels of learned transfers; the
banded line solves are symmetric when A is, so the cycle stays a symmetric operator.
precond_gs_mode (smoothing.GS_MODES, Gauss-Seidel only): the ordering of the sweeps.  "multicolor_device" runs the colours
forward before and in reverse after the coarse correction -- the symmetric multicolour cycle, with the colouring and the
colour-ordered sliced-ELL copy of every level made on the device."""
import math

import numpy as np
import torch

from .. import ops
from ..ops import F64
from ._precond import BlockSolves, check_smoother, gs_mode_keyword, make_apply
from .Solver import IterativeSolver, on_device


class CG(BlockSolves, IterativeSolver):

    def __init__(self, matrix, rhs, **kw):
        super().__init__(matrix, rhs, **kw)
        self._log("Selected CG")
        self.label = "CG"
        self._reset_blocks()               # solve_many's caches

    @on_device
    def solve(self, max_iterations=1000, error=1e-08, initial_guess=None, *, preconditioner=None,
              precond_steps=2, precond_omega=0.8, precond_smoother="Jacobi", precond_cycle_shape="V",
              precond_line_dir="xy", precond_line_order="zebra", precond_line_band=None,
              precond_gs_mode="lexicographic"):
        gs_mode_keyword(precond_gs_mode)
        options = check_smoother(precond_smoother, precond_steps, line_dir=precond_line_dir, line_order=precond_line_order,
                                 line_band=precond_line_band)
        if precond_cycle_shape not in ("V", "W"):
            raise ValueError("precond_cycle_shape must be 'V' or 'W' (CG needs a symmetric preconditioner), got %r"
                             % (precond_cycle_shape,))
        A = self._device_matrix()
        A.pack()
        n = self.dim
        dev = self._device
        b = self._to_device(self.rhs)
        x = torch.zeros(n, dtype=F64, device=dev) if initial_guess is None else self._to_device(initial_guess)
        r = torch.empty_like(x)
        Ap = torch.empty_like(x)
        part = torch.empty(ops.partials_count(n), dtype=F64, device=dev)
        s = torch.zeros(1, dtype=F64, device=dev)
        ops.csr_residual_norm2(A, x, b, r, part, s)                    # CG.py:21-22
        self.residual = math.sqrt(s.item())
        track = [self.residual]
        H = preconditioner
        # forward sweeps before, backward sweeps after the coarse correction: the symmetric Gauss-Seidel cycle
        apply_M = make_apply(H, precond_smoother, precond_steps, precond_omega, precond_cycle_shape, ("forward", "backward"),
                             options, **gs_mode_keyword(precond_gs_mode))
        z = torch.empty_like(x)
        apply_M(r, z)
        p = z.clone()
        ops.dot(r, z, part, s)
        rz = s.item()
        for _ in range(max_iterations):
            self.iterations += 1
            ops.csr_spmv(A, p, Ap, 1.0, 0.0)                           # :31
            ops.dot(p, Ap, part, s)
            pAp = s.item()
            alpha = rz / pAp                                           # :34
            ops.axpby(alpha, p, 1.0, x)                                # :35
            ops.axpby(-alpha, Ap, 1.0, r)                              # :37
            ops.dot(r, r, part, s)
            self.residual = math.sqrt(s.item())                        # :41
            track.append(self.residual)
            if self.residual <= error:
                self._log("Reached convergence")
                break
            apply_M(r, z)
            if H is None:
                rz_new = s.item()
            else:
                ops.dot(r, z, part, s)
                rz_new = s.item()
            beta = rz_new / rz                                         # :47
            rz = rz_new
            ops.axpby(1.0, z, beta, p)                                 # :48
        if H is not None and precond_smoother == "GaussSeidel":
            H.check_smoothers()            # a timed-out wavefront band raises instead of leaving a wrong solution
        self.solution = self._column(x)
        self.residual_vector = self._column(r)
        self.track_res = np.array(track, dtype=float).reshape(-1, 1)

    # -- several right-hand sides at once (no counterpart in the reference) ----------------------
    @on_device
    def solve_many(self, rhs, max_iterations=1000, error=1e-08, initial_guess=None, *, preconditioner=None,
                   precond_steps=2, precond_omega=0.8, precond_cycle_shape="V", use_graph=False):
        """Solve A X = rhs for the m >= 1 columns of rhs (n, m) by (multigrid-preconditioned) conjugate gradients on
        blocks of columns (krylov.block_pcg): the operator and, with preconditioner=Hierarchy, every matrix of the
        hierarchy are read once per iteration for up to 8 columns, and alpha, beta and the convergence test of every column
        stay on the device -- one device-to-host read of 2 k doubles per iteration.  Every column runs its own CG recurrence;
        a column whose recurrence norm is <= error is frozen: its solution is, bit for bit, the iterate of the iteration at
        which it passed, while the other columns of its chunk go on.
        Columns are padded with zero columns to a width of 2, 4 or 8 and worked through in chunks of 8, like
        Multigrid.solve_many.  Returns (X, track): X (n, m); track row 0 holds the true ||b_j - A x_j||_2 of the initial
        guess, every further row one iteration's recurrence norm sqrt(r_j . r_j) -- NaN after the iteration at which the
        column passed, and in rows that its chunk did not reach because another chunk needed more.
        self.iterations_many[j]: the iterations column j ran (0: it started at or below error).
        The preconditioner is one precond_cycle_shape ("V" | "W") cycle of block.BlockCycle from a zero guess, which smooths
        with weighted Jacobi only (precond_steps sweeps before and after, damping precond_omega): no other smoother can
        be asked for here.  A hierarchy with cycle_values="f32" is refused by BlockCycle.  use_graph replays the cycle
        from a captured hipGraph; everything else of an iteration is launched as it is.  solve() is not touched by any of
        this."""
        if precond_cycle_shape not in ("V", "W"):
            raise ValueError("precond_cycle_shape must be 'V' or 'W' (CG needs a symmetric preconditioner), got %r"
                             % (precond_cycle_shape,))
        from .. import krylov

        def columns(A, block_cycle, B, X0, dev):
            return krylov.block_pcg_columns(ops, A, block_cycle, B, X0, dev, max_iterations=int(max_iterations), error=error,
                                            steps=precond_steps, omega=precond_omega, shape=precond_cycle_shape,
                                            use_graph=bool(use_graph))

        return self._solve_many(rhs, initial_guess, preconditioner, columns)
