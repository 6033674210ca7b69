"""Multigrid cycles on a block of right-hand sides: one pass over every matrix of the hierarchy for k columns.

On a hierarchy of learned or L2-type transfer operators the cycle is bound by the matrix bytes it streams (25- and
49-entry Galerkin rows with all-distinct values, DESIGN.md sections 3 and 7).  Someone who solves the same operator for
several right-hand sides pays those bytes once per column with solve(); BlockCycle pays them once per k columns: every
level's A, P and R get an fp64 sliced-ELL twin (ops.block_twin) and every sweep is one lmg_sell_sweep_block launch on
(n, k) blocks, k in ops.BLOCK_WIDTHS.  Column j of every launch carries the bits of the single-vector SELL sweep on that
column, so a block cycle is k independent cycles that share their matrix traffic.

Weighted Jacobi only; fp64 values only (a hierarchy with cycle_values="f32" is refused).  On constant-coefficient grid
hierarchies the single-vector fused passes read one byte of matrix per row and this path has nothing to amortise: there,
k calls of solve() are faster.
"""
import math

import torch

from .hierarchy import capture_cycle, cycle_children, linear_cycle_children
from .ops import F64


def block_width(ncols, widths):
    """The narrowest width that holds ncols columns (the widest for more: the caller works in chunks of it)."""
    for k in widths:
        if ncols <= k:
            return k
    return widths[-1]


class _BlockLevel:
    __slots__ = ("n", "A", "P", "R", "x", "b", "r", "tmp", "shared_A")


class BlockCycle:
    """The cycle of a finished Hierarchy H on blocks of up to nrhs columns (padded with zero columns to the next width
    in ops.BLOCK_WIDTHS; a single column runs at the narrowest).  levels[0].x / .b are the fine blocks, (n, k) tensors
    the caller fills; columns nrhs .. k-1 stay zero through every kernel.  Everything is allocated here, nothing later:
    a cycle can be captured into a hipGraph (captured()).
    What is derived from the values of H -- the twins of every level's A that are not the matrix's own, the captured
    cycles, which coarse solver there is -- follows H.rebuild_numeric(): every public method compares H.generation first
    (_sync) and gives what a BlockCycle built after the rebuild gives.  (The one allocation after construction: the two
    column vectors, when a rebuild leaves H with a coarse solver that has no block form.)"""

    def __init__(self, H, nrhs):
        if getattr(H, "cycle_values", "f64") != "f64":
            raise ValueError("BlockCycle needs a hierarchy with cycle_values='f64': the block sweeps read fp64 values (a "
                             "hierarchy with cycle_values=%r is a preconditioner for CG / GMRES)" % (H.cycle_values,))
        self.H = H
        self.ops = ops_ = H.ops
        widths = tuple(ops_.BLOCK_WIDTHS)
        nrhs = int(nrhs)
        if not 1 <= nrhs <= widths[-1]:
            raise ValueError("a block holds 1 .. %d right-hand sides, got %d" % (widths[-1], nrhs))
        self.nrhs = nrhs
        self.k = k = block_width(nrhs, widths)
        dev = H.device
        self.levels = []
        for lev in H.levels:
            bl = _BlockLevel()
            bl.n = lev.n
            bl.A = ops_.block_twin(lev.A)
            # the matrix's own fp64 twin (repack_values keeps it current), or a copy of the values that _sync rewrites
            bl.shared_A = bl.A is getattr(lev.A, "sell", None)
            bl.P = None if lev.P is None else ops_.block_twin(lev.P)
            bl.R = None if lev.R is None else ops_.block_twin(lev.R)
            bl.x, bl.b, bl.r, bl.tmp = (torch.zeros((lev.n, k), dtype=F64, device=dev) for _ in range(4))
            self.levels.append(bl)
        self.partials = torch.empty(ops_.block_partials_count(self.levels[0].n, k), dtype=F64, device=dev)
        self.norm2 = torch.zeros(k, dtype=F64, device=dev)
        self.col_b = self.col_x = None
        self._coarse_kind()
        self._graphs = {}
        self._generation = getattr(H, "generation", 0)

    def _coarse_kind(self):
        """Which coarse solver H has now, and the vectors of the column loop where it has no block form."""
        self.dense_coarse = getattr(self.H.coarse, "kind", None) == "dense"
        if not self.dense_coarse and self.col_b is None:
            # the column loop of a coarse solver without a block form: one right-hand side and one solution at a time
            nc, dev = self.levels[-1].n, self.H.device
            self.col_b = torch.zeros(nc, dtype=F64, device=dev)
            self.col_x = torch.zeros(nc, dtype=F64, device=dev)

    def _sync(self):
        """Follow H.rebuild_numeric(): nothing to do while H.generation is what it was.  After a rebuild every level's A has
        new values on the same pattern (P and R have not changed): a twin that was the matrix's own is asked for again
        (repack_values may have put another object there), a twin of this cycle's own gets the new value stream in place.
        The captured cycles hold the addresses of the old coarse inverse and are dropped; the coarse solver may be one of
        another kind.  Never runs inside a capture: captured() has called it before."""
        gen = getattr(self.H, "generation", 0)
        if gen == self._generation:
            return
        for bl, lev in zip(self.levels, self.H.levels):
            if bl.shared_A or not hasattr(bl.A, "update_values"):    # (not a twin at all: the CPU stand-ins hand out the matrix)
                bl.A = self.ops.block_twin(lev.A)
                bl.shared_A = bl.A is getattr(lev.A, "sell", None)
            elif not bl.A.update_values(lev.A):
                raise RuntimeError("the block twin of a level with %d rows refused its new values" % bl.n)
        self._graphs = {}
        self._coarse_kind()
        self._generation = gen

    def use_columns(self, nrhs):
        """Start over with nrhs columns of the same width: the fine iterate and right-hand side are cleared (the caller
        fills columns 0 .. nrhs-1; the others must stay zero)."""
        nrhs = int(nrhs)
        if nrhs < 1 or block_width(nrhs, tuple(self.ops.BLOCK_WIDTHS)) != self.k:
            raise ValueError("%d columns do not belong in a block of width %d" % (nrhs, self.k))
        self._sync()
        self.nrhs = nrhs
        # (the coarsest blocks too: the column loop of a coarse solver without a block form writes nrhs columns only)
        for t in (self.levels[0].x, self.levels[0].b, self.levels[-1].x, self.levels[-1].tmp):
            self.ops.zero(t.view(-1))

    # ------------------------------------------------------------------ the cycle ------
    def _smooth(self, bl, steps, omega):
        for _ in range(steps):
            self.ops.block_jacobi(bl.A, bl.x, bl.b, omega, bl.tmp)
            bl.x, bl.tmp = bl.tmp, bl.x

    def _coarse_apply(self, B, X):
        """X = A_L^-1 B: one product with the dense inverse, or the hierarchy's solver column by column."""
        if self.dense_coarse:
            self.ops.dense_gemv_block(self.H.coarse.inv, B, X)
            return
        for j in range(self.nrhs):                                   # (zero columns of X stay as they are: zero)
            self.ops.copy2d(B[:, j:j + 1], self.col_b.view(-1, 1))
            self.H.coarse.apply(self.col_b, self.col_x)
            self.ops.copy2d(self.col_x.view(-1, 1), X[:, j:j + 1])

    def _coarse_solve(self):
        bl = self.levels[-1]
        self._coarse_apply(bl.b, bl.x)
        for _ in range(self.H.coarse_refine):
            self.ops.block_residual_norm2(bl.A, bl.x, bl.b, bl.r, None, None)
            self._coarse_apply(bl.r, bl.tmp)
            self.ops.axpby(1.0, bl.tmp.view(-1), 1.0, bl.x.view(-1))

    def _visit(self, l, children, steps, omega):
        bl, nxt = self.levels[l], self.levels[l + 1]
        self._smooth(bl, steps, omega)
        self.ops.block_residual_norm2(bl.A, bl.x, bl.b, bl.r, None, None)
        self.ops.block_spmv(bl.R, bl.r, nxt.b, 1.0, 0.0)
        if l + 2 == len(self.levels):
            self._coarse_solve()
        else:
            self.ops.zero(nxt.x.view(-1))
            for sub in children:                       # a second visit starts from the first one's iterate, same b
                self._visit(l + 1, cycle_children(sub), steps, omega)
        self.ops.block_spmv(bl.P, nxt.x, bl.x, 1.0, 1.0)
        self._smooth(bl, steps, omega)

    def cycle(self, steps, omega, shape="V"):
        """One V(steps, steps), W or F cycle (the linear shapes of Hierarchy.cycle; "K" raises ValueError) with weighted
        Jacobi on levels[0].x / .b."""
        children = linear_cycle_children(shape, "BlockCycle")
        self._sync()
        self._visit(0, children, int(steps), float(omega))

    def apply(self, src, dst, steps, omega, shape="V", use_graph=False):
        """One cycle on the right-hand sides src (an (n, k) block) from a zero guess: the cycle as a preconditioner.  The
        result is levels[0].x, which is returned; dst (None: no copy) receives a copy of it.  use_graph: the cycle itself
        is the replay of captured()."""
        self._sync()
        fine = self.levels[0]
        self.ops.copy(src.view(-1), fine.b.view(-1))
        self.ops.zero(fine.x.view(-1))
        if use_graph:
            self.captured(steps, omega, shape).launch()
        else:
            self.cycle(steps, omega, shape)
        out = self.levels[0].x
        if dst is not None:
            self.ops.copy(out.view(-1), dst.view(-1))
        return out

    def residual_norms(self):
        """||b_j - A x_j||_2 of the nrhs columns on the fine level: one block residual, one read of k doubles."""
        self._sync()
        bl = self.levels[0]
        self.ops.block_residual_norm2(bl.A, bl.x, bl.b, None, self.partials, self.norm2)
        return [math.sqrt(max(v, 0.0)) for v in self.norm2.cpu().tolist()[:self.nrhs]]

    def captured(self, steps, omega, shape="V"):
        """The launch sequence of cycle(), captured once into a hipGraph on H.stream's capture and replayed."""
        self._sync()                                   # (before the capture: cycle() inside it finds nothing to do)
        key = (int(steps), float(omega), shape, self.nrhs)
        g = self._graphs.get(key)
        if g is None:
            linear_cycle_children(shape, "BlockCycle")
            g = self._graphs[key] = capture_cycle(self.ops, self.levels, lambda: self.cycle(steps, omega, shape))
        return g
