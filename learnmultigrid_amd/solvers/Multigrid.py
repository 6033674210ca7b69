"""Multigrid V-cycle solvers with the reference's call signatures
(learn_multigrid/solvers/Multigrid.py:26-197), executed on an MI355X.

    GeometricMG(A, rhs).solve(levels=3, smoother="GaussSeidel", smooth_steps=3, ...)
    SemiGeometricMG(A, rhs, Q).solve(levels=2, smoother="GaussSeidel", smooth_steps=3,
                                     error=1e-10, max_iterations=40)
    mg.get_track_res(), mg.get_iterations(), mg.get_solution(), mg.get_residual()

Reference behaviour that is reproduced on purpose:
  * the first recorded residual is ||1|| = sqrt(n) (Multigrid.py:64-66);
  * convergence is tested BEFORE each cycle; `iterations` counts started iterations;
  * `levels` counts grids (levels-1 coarsenings, direct solve on the last, :78,:102);
  * as shipped, the `smoother` name is ignored and forward lexicographic Gauss-Seidel
    is always applied (:79-88,:121): that is `smoother_semantics="as_shipped"`, the
    default.  `smoother_semantics="as_named"` honours the name ("Jacobi" with `omega`,
    "GaussSeidel" with `gs_mode`), which is what the commented-out lines :85-86 intend;
  * SemiGeometricMG uses the supplied Q between levels 0 and 1 only and the 1-D
    geometric interpolator below (:188-197) unless a `hierarchy` list is given.
Deviations (all louder, none silent): unknown cycle / smoother / levels < 2 raise
ValueError instead of sys.exit(0) / TypeError / unbounded recursion; printing is
opt-in (verbose=True); the caller's initial_guess is only overwritten when
mutate_initial_guess=True (the reference smooths it in place, :43,:88).
What the reference recomputes in every cycle (transfer lookup, R A P, SuperLU
factorisation) is done once per solve() in the Hierarchy setup.
"""
import numpy as np
import scipy.sparse as sp
import torch

from .. import krylov, ops, problems
from ..hierarchy import KRYLOV_SHAPES, Hierarchy, cycle_children, gs_sweep_pair, k_inner_name, linear_cycle_children
from ..smoothing import smoother_options
from ._precond import BlockSolves, check_columns, hierarchy_stream
from .Solver import IterativeSolver, on_device

_SMOOTHERS = ("GaussSeidel", "Jacobi", "CG")          # Multigrid.py:149-155
_EXTRA_SMOOTHERS = ("Chebyshev", "Line")                    # not in the reference: honoured under smoother_semantics="as_named"


class Multigrid(BlockSolves, IterativeSolver):

    def __init__(self, matrix, rhs, **kw):
        super().__init__(matrix, rhs, **kw)
        self._log("Selected Multigrid")
        self.label = "Multigrid"
        self.hierarchy = None              # optional list of transfer operators (all levels)
        self._hier = None
        self._hier_key = None
        self._reset_blocks()               # solve_many's cache of block cycles

    # -- transfer-operator dispatch (Multigrid.py:91 -> :126 / :171 / :188) --------------------
    def interpolator(self, dimension, _first_call=False):
        """1-D geometric interpolator (n x floor((n-1)/2)+1), CSR with the values of
        Multigrid.py:126-147 (the reference returns the same matrix dense)."""
        return problems.geometric_interpolator_1d(dimension)

    def _transfers(self, levels, first_call):
        n = self.dim
        out = []
        for l in range(levels - 1):
            if self.hierarchy is not None:
                if l >= len(self.hierarchy):
                    raise ValueError("hierarchy has %d operators, levels=%d needs %d"
                                     % (len(self.hierarchy), levels, levels - 1))
                P = sp.csr_matrix(self.hierarchy[l])
            else:
                P = self.interpolator(n, first_call if l == 0 else False)   # :103-104
            if P.shape[0] != n:
                raise ValueError("transfer operator %d has %d rows, expected %d" % (l, P.shape[0], n))
            out.append(P)
            n = P.shape[1]
        return out

    def _setup(self, levels, first_call, coarse_refine):
        key = (levels, bool(first_call), id(self.matrix), str(coarse_refine),
               None if self.hierarchy is None else tuple(id(h) for h in self.hierarchy))
        if self._hier is None or self._hier_key != key:
            self._hier = Hierarchy(self.matrix, self._transfers(levels, first_call), self._device,
                                   coarse_refine=coarse_refine, verbose=self.verbose)
            self._hier_key = key
        return self._hier

    def _invalidate(self):
        super()._invalidate()
        self._hier = None

    @staticmethod
    def _effective_smoother(smoother, semantics):
        if smoother not in _SMOOTHERS + _EXTRA_SMOOTHERS:
            raise ValueError("unknown smoother %r (reference: 'Jacobi', 'GaussSeidel', 'CG'; this build also: 'Chebyshev', 'Line')"
                             % (smoother,))
        if semantics == "as_shipped":
            return "GaussSeidel"
        if semantics != "as_named":
            raise ValueError("smoother_semantics must be 'as_shipped' or 'as_named'")
        if smoother == "CG":
            raise ValueError("CG is not a V-cycle smoother in this build (unused by the reference too)")
        return smoother

    def _ready(self, H, eff, options):
        """Prepare H for the smoother as its options ask (smoother_options); one without any sets itself up in its first sweep."""
        if options:
            H.prepare_smoother(eff, **options)

    # -- Multigrid.solve (Multigrid.py:36-75) ---------------------------------------------------
    @on_device
    def solve(self, levels=2, smoother="Jacobi", smooth_steps=1, max_iterations=100, error=1e-08,
              initial_guess=None, cycle="V", first_call=False, *, omega=1.0,
              smoother_semantics="as_shipped", gs_mode="lexicographic", coarse_refine="auto",
              use_graph=False, mutate_initial_guess=False, gs_sweep="forward", cycle_shape="V",
              cheby_lmax=None, cheby_ratio=None, line_dir="xy", line_order="zebra", line_band=None, k_inner="gcr"):
        """smoother="Line" (under smoother_semantics="as_named"; as shipped the name is ignored like every other): line
        relaxation -- smooth_steps steps with damping omega before and after the coarse correction, each solving the
        tridiagonal systems of the grid lines in direction line_dir ("x": storage lines, "y": grid columns, "xy": x then y;
        the post-smoothing half runs the reverse order), even systems then odd ones (line_order="zebra", omega = 1.0 suits)
        or all from one residual (line_order="jacobi", omega ~ 0.8).  The smoother for operators with a strong direction;
        grid levels with a 3x3 stencil only unless line_band (1 | 2 | 3, None = 1) allows the wider lines of 25-point (2) and
        49-point (3) Galerkin levels (Hierarchy.prepare_smoother, which also says which level cannot run it, and why).
        smoother="Chebyshev" (under smoother_semantics="as_named"; as shipped the name is ignored like every other): one
        Chebyshev polynomial smoothing step of degree smooth_steps on D^-1 A before and after the coarse correction, on
        [lmax / cheby_ratio, lmax] per level.  cheby_lmax: None = each level's Gershgorin bound, a float, or one value per
        smoothed level; cheby_ratio: None = 4.0 (Hierarchy.prepare_smoother).  omega is not used.
        gs_sweep: direction of the Gauss-Seidel smoothing (also under as_shipped semantics, where Gauss-Seidel always
        runs) -- a pyamg sweep name ("forward" | "backward" | "symmetric") for pre- and post-smoothing, or a (pre, post)
        pair.  ("forward", "backward") gives a symmetric V-cycle at one pipelined launch per smoothing half; "symmetric"
        costs a launch per direction and step.
        cycle_shape: "V" | "W" | "F", what pyamg's cycle= selects, or "K", the Krylov-accelerated cycle (pyamg's 'AMLI';
        Hierarchy.cycle): every coarse visit is two steps of k_inner = "gcr" (any operator, the default) or "fcg" (symmetric
        positive definite operators and symmetric cycles) preconditioned by the cycle below, at the cost of a W-cycle; for
        hierarchies that coarsen aggressively.  `cycle` keeps the reference's V-only switch (:55-57)."""
        if cycle != "V":
            raise ValueError("Cycle type unknown: %r" % (cycle,))            # :55-57
        if levels < 2:
            raise ValueError("levels must be >= 2 (levels counts grids)")
        eff = self._effective_smoother(smoother, smoother_semantics)
        pair = gs_sweep_pair(gs_sweep)
        cycle_children(cycle_shape)
        k_inner_name(k_inner)
        options = smoother_options(eff, smooth_steps, cheby_lmax=cheby_lmax, cheby_ratio=cheby_ratio, line_dir=line_dir,
                                   line_order=line_order, line_band=line_band)
        H = self._setup(levels, first_call, coarse_refine)
        with hierarchy_stream(H, self._device):
            self._ready(H, eff, options)
            self._solve_on_stream(H, eff, smooth_steps, max_iterations, error, initial_guess, omega,
                                  gs_mode, use_graph, mutate_initial_guess, pair, cycle_shape, k_inner)

    def _solve_on_stream(self, H, eff, smooth_steps, max_iterations, error, initial_guess, omega,
                         gs_mode, use_graph, mutate_initial_guess, gs_sweep=("forward", "forward"), shape="V", k_inner="gcr"):
        krylov_kw = {"k_inner": k_inner} if shape in KRYLOV_SHAPES else {}
        fine = H.levels[0]
        if initial_guess is None:
            self._log("You should put an initial guess. Used zero vector")
            ops.zero(fine.x)
        else:
            fine.x.copy_(self._to_device(initial_guess))
        fine.b.copy_(self._to_device(self.rhs))
        hook = None
        if mutate_initial_guess and initial_guess is not None:
            state = {"done": False}

            def hook(x_dev):
                if not state["done"]:
                    np.asarray(initial_guess).reshape(-1)[:] = x_dev.cpu().numpy()
                    state["done"] = True
        graph = H.captured_cycle(eff, smooth_steps, omega, gs_mode, gs_sweep, shape, **krylov_kw) if use_graph else None
        track = []
        for _ in range(max_iterations):                                      # :59
            self.iterations += 1
            self.residual = H.residual_norm()                                # :62-63
            if eff == "GaussSeidel":
                H.check_smoothers()          # the norm read has synchronised: a timed-out wavefront band raises here
            if self.iterations <= 1:                                         # :64-66
                self.residual = float(np.linalg.norm(np.ones(shape=(self.dim, 1))))
            track.append(self.residual)
            self._log("It: ", self.iterations, self.residual)
            if self.residual <= error:                                       # :69-71
                break
            if graph is not None and hook is None:
                graph.launch()
            else:
                H.cycle(eff, smooth_steps, omega, gs_mode, after_presmooth=hook, gs_sweep=gs_sweep, shape=shape,
                        **krylov_kw)                                                                        # :73
                hook = None
        self.solution = self._column(fine.x)
        self.residual_vector = (np.ones(shape=(self.dim, 1)) if self.iterations <= 1
                                else self._column(H.outer_r))
        self.track_res = np.array(track, dtype=float).reshape(-1, 1)         # :75
        self.level_dims = H.sizes

    # -- several right-hand sides at once (no counterpart in the reference) ----------------------
    _FIRST_CALL = False            # the first_call solve() defaults to: solve_many shares solve()'s cached hierarchy

    @on_device
    def solve_many(self, rhs, levels=2, smooth_steps=1, max_iterations=100, error=1e-08, initial_guess=None, *,
                   omega=1.0, cycle_shape="V", coarse_refine="auto", use_graph=False, smoother="Jacobi"):
        """Solve A X = rhs for the m >= 1 columns of rhs (n, m) with one multigrid cycle per iteration on all of them:
        every sweep reads its matrix once for up to 8 columns (block.BlockCycle) instead of once per column -- what pays
        on hierarchies of learned or L2-type transfers, whose levels stream 25- and 49-entry rows; on constant-coefficient
        grid hierarchies m calls of solve() are faster.  Returns (X, track): X (n, m), and
        track (iterations, m), the true residual norms ||b_j - A x_j||_2 taken before each cycle -- no sqrt(n) first
        entry, that quirk belongs to the reference's solve().
        The smoother is weighted Jacobi with `omega`, smooth_steps sweeps before and after the coarse correction: this is
        smoother_semantics="as_named" with smoother="Jacobi" (any other smoother raises ValueError), cycle_shape "V" | "W" |
        "F" as in solve() ("K" raises ValueError: the block cycle has no K-cycle).  Column j carries the bits of a
        single-vector sliced-ELL cycle on column j.
        Columns are padded with zero columns to a width of 2, 4 or 8 and worked through in chunks of 8.  All columns of
        a chunk iterate until every one is <= error or max_iterations is reached: a column that has passed is not
        deflated, it simply keeps being smoothed (its residual keeps falling and is still recorded).
        self.iterations_many[j]: the number of cycles before column j first passed, or max_iterations.  Rows of track
        beyond the last iteration of a column's chunk (another chunk needed more) hold NaN."""
        B, X0 = check_columns(rhs, initial_guess, self.dim)
        if levels < 2:
            raise ValueError("levels must be >= 2 (levels counts grids)")
        if smoother != "Jacobi":
            raise ValueError("solve_many smooths with weighted Jacobi only, got smoother=%r" % (smoother,))
        linear_cycle_children(cycle_shape, "Multigrid.solve_many")
        H = self._setup(levels, self._FIRST_CALL, coarse_refine)

        def solve_chunk(bc, Bk, Xk, mc):
            graph = bc.captured(smooth_steps, omega, cycle_shape) if use_graph else None
            rows, its = [], np.full(mc, int(max_iterations), dtype=np.int64)
            for it in range(int(max_iterations)):
                norms = np.array(bc.residual_norms())
                rows.append(norms)
                passed = norms <= error
                its[passed & (its == max_iterations)] = it
                self._log("It: ", it + 1, norms)
                if passed.all():
                    break
                if graph is not None:
                    graph.launch()
                else:
                    bc.cycle(smooth_steps, omega, cycle_shape)
            return rows, its

        with hierarchy_stream(H, self._device):
            X, track, self.iterations_many = krylov.columns_in_chunks(ops, lambda mc: self._block_cycle(H, mc), B, X0,
                                                                      self._device, solve_chunk, in_cycle=True)
        self.level_dims = H.sizes
        return X, track

    # -- Multigrid.v_cycle (Multigrid.py:77) ------------------------------------------------------
    @on_device
    def v_cycle(self, A, u0, rhs, smoother, smooth_steps, error, levels, first_call=False, *,
                omega=1.0, smoother_semantics="as_shipped", gs_mode="lexicographic",
                coarse_refine="auto", gs_sweep="forward", cheby_lmax=None, cheby_ratio=None, line_dir="xy",
                line_order="zebra", line_band=None):
        """One V-cycle on (A, rhs) from u0; returns a fresh (n,1) array.  u0 receives the
        pre-smoothed iterate like in the reference (:88-89).  gs_sweep, cheby_lmax, cheby_ratio, line_dir, line_order, line_band
        as in solve()."""
        return self._one_cycle("V", A, u0, rhs, smoother, smooth_steps, levels, first_call, omega, smoother_semantics,
                               gs_mode, coarse_refine, gs_sweep, cheby_lmax, cheby_ratio, line_dir, line_order, line_band)

    @on_device
    def w_cycle(self, A, u0, rhs, smoother, smooth_steps, error, levels, first_call=False, *,
                omega=1.0, smoother_semantics="as_shipped", gs_mode="lexicographic",
                coarse_refine="auto", gs_sweep="forward", cheby_lmax=None, cheby_ratio=None, line_dir="xy",
                line_order="zebra", line_band=None):
        """One W-cycle (solve(cycle_shape="W")) with v_cycle's arguments and behaviour."""
        return self._one_cycle("W", A, u0, rhs, smoother, smooth_steps, levels, first_call, omega, smoother_semantics,
                               gs_mode, coarse_refine, gs_sweep, cheby_lmax, cheby_ratio, line_dir, line_order, line_band)

    @on_device
    def f_cycle(self, A, u0, rhs, smoother, smooth_steps, error, levels, first_call=False, *,
                omega=1.0, smoother_semantics="as_shipped", gs_mode="lexicographic",
                coarse_refine="auto", gs_sweep="forward", cheby_lmax=None, cheby_ratio=None, line_dir="xy",
                line_order="zebra", line_band=None):
        """One F-cycle (solve(cycle_shape="F")) with v_cycle's arguments and behaviour."""
        return self._one_cycle("F", A, u0, rhs, smoother, smooth_steps, levels, first_call, omega, smoother_semantics,
                               gs_mode, coarse_refine, gs_sweep, cheby_lmax, cheby_ratio, line_dir, line_order, line_band)

    @on_device
    def k_cycle(self, A, u0, rhs, smoother, smooth_steps, error, levels, first_call=False, *,
                omega=1.0, smoother_semantics="as_shipped", gs_mode="lexicographic",
                coarse_refine="auto", gs_sweep="forward", cheby_lmax=None, cheby_ratio=None, line_dir="xy",
                line_order="zebra", line_band=None, k_inner="gcr"):
        """One K-cycle (solve(cycle_shape="K", k_inner=...)) with v_cycle's arguments and behaviour."""
        return self._one_cycle("K", A, u0, rhs, smoother, smooth_steps, levels, first_call, omega, smoother_semantics,
                               gs_mode, coarse_refine, gs_sweep, cheby_lmax, cheby_ratio, line_dir, line_order, line_band,
                               k_inner=k_inner_name(k_inner))

    def _one_cycle(self, shape, A, u0, rhs, smoother, smooth_steps, levels, first_call, omega, smoother_semantics,
                   gs_mode, coarse_refine, gs_sweep, cheby_lmax, cheby_ratio, line_dir, line_order, line_band, **krylov_kw):
        if levels < 2:
            raise ValueError("levels must be >= 2")
        eff = self._effective_smoother(smoother, smoother_semantics)
        pair = gs_sweep_pair(gs_sweep)
        options = smoother_options(eff, smooth_steps, cheby_lmax=cheby_lmax, cheby_ratio=cheby_ratio, line_dir=line_dir,
                                   line_order=line_order, line_band=line_band)
        if A is self.matrix:
            H = self._setup(levels, first_call, coarse_refine)
        else:
            saved = self.matrix, self.dim, self._hier, self._hier_key
            self.matrix, self.dim = sp.csc_matrix(A), A.shape[0]
            self._hier = None
            try:
                H = self._setup(levels, first_call, coarse_refine)
            finally:
                self.matrix, self.dim, self._hier, self._hier_key = saved
        fine = H.levels[0]
        n = fine.n
        u0a = np.asarray(u0)
        fine.x.copy_(torch.from_numpy(np.ascontiguousarray(u0a, dtype=np.float64).reshape(-1)).to(self._device))
        fine.b.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(rhs), dtype=np.float64).reshape(-1)).to(self._device))

        def hook(x_dev):
            if u0a.dtype == np.float64 and u0a.flags.writeable:
                u0a.reshape(-1)[:] = x_dev.cpu().numpy()
        with hierarchy_stream(H, self._device):
            self._ready(H, eff, options)
            H.cycle(eff, smooth_steps, omega, gs_mode, after_presmooth=hook, gs_sweep=pair, shape=shape, **krylov_kw)
            out = fine.x.cpu().numpy().reshape(n, 1).copy()
            if eff == "GaussSeidel":
                H.check_smoothers()
        return out

    def smoother_to_method(self, smoother):
        from .Jacobi import Jacobi
        from .GaussSeidel import GaussSeidel
        table = {"GaussSeidel": GaussSeidel, "Jacobi": Jacobi}
        if smoother not in table:
            raise ValueError("Invalid smoother %r" % (smoother,))
        return table[smoother]

    def cycle_to_method(self, cycle):
        if cycle != "V":
            raise ValueError("Invalid cycle %r" % (cycle,))
        return self.v_cycle


class GeometricMG(Multigrid):
    """Multigrid.py:164-173: 1-D geometric interpolator on every level."""

    def __init__(self, matrix, rhs, **kw):
        super().__init__(matrix, rhs, **kw)
        self._log("Selected Geometric Multigrid")
        self.label = "GeometricMG"


class SemiGeometricMG(Multigrid):
    """Multigrid.py:176-197: l2_proj (any matrix with one row per fine unknown -- an L2
    projection or a learned Q) between levels 0 and 1, geometric below.  `hierarchy`
    (keyword-only) supplies the operators of ALL levels instead: the consumer that
    NeuralMG_2D.define_hierarchy's l_hierarchy (Multigrid.py:741-765) never had."""

    def __init__(self, matrix, rhs, l2_proj, *, hierarchy=None, **kw):
        super().__init__(matrix, rhs, **kw)
        self._log("Selected Semi - Geometric Multigrid")
        self.label = "SemiGeometricMG"
        self.l2_proj = sp.csr_matrix(l2_proj)                               # :182
        if hierarchy is not None:
            self.hierarchy = [sp.csr_matrix(h) for h in hierarchy]

    _FIRST_CALL = True

    def solve(self, levels=2, smoother="Jacobi", smooth_steps=1, max_iterations=100, error=1e-08,
              initial_guess=None, cycle="V", first_call=True, **kw):       # :184-186
        super().solve(levels, smoother, smooth_steps, max_iterations, error, initial_guess, cycle,
                      first_call, **kw)

    def interpolator(self, dimension, first_call=False):                    # :188-197
        if first_call:
            return self.l2_proj
        return super().interpolator(dimension, first_call)


class HierarchyMG(SemiGeometricMG):
    """Convenience spelling: HierarchyMG(A, rhs, [Q0, Q1, ...]) == SemiGeometricMG with
    hierarchy=[...] (one learned / projected transfer operator per coarsening)."""

    def __init__(self, matrix, rhs, hierarchy, **kw):
        hierarchy = list(hierarchy)
        super().__init__(matrix, rhs, hierarchy[0], hierarchy=hierarchy, **kw)
        self.label = "HierarchyMG"


class NeuralMG(Multigrid):
    """Multigrid.py:200-370: `NeuralMG(matrix, rhs, model, M, std, mean)`.  The transfer operator of
    every level is built from that level's mass matrix by the caller's model
    (`model.predict`, any object; see learned_q.py for the scatter) and the mass matrix is
    coarsened with it, M_c = Q^T M Q (:273-275).  The reference asks the model again in every
    cycle; a deterministic model returns the same Q each time, so the operators are built once
    per solve() here (setup / solve split) and the cycles run on the device."""

    def __init__(self, matrix, rhs, model, M, std, mean, **kw):
        super().__init__(matrix, rhs, **kw)
        self._log("Selected NN Multigrid")
        self.label = "NeuralMG"
        self.model, self.M, self.std, self.mean = model, M, std, mean

    def transfer_op(self, M):
        from ..learned_q import learned_transfer
        return learned_transfer(self.model, M, self.mean, self.std)                 # :306-311

    def _transfers(self, levels, first_call):
        out = []
        M = sp.csr_matrix(self.M)
        for _ in range(levels - 1):
            if M.shape[0] % 2 == 0:
                raise ValueError("mass matrix of even size %d: the learned 1-D transfer needs odd sizes "
                                 "(test/test_B_patch.py:52-53)" % M.shape[0])
            Q = sp.csr_matrix(self.transfer_op(np.asarray(M.toarray())))
            out.append(Q)
            # M_coarse = Q^T M Q (:273-275) by the device SpGEMM, evaluated (Q^T M) Q like SciPy does: the
            # same bits as the host product without forming dense n x n matrices for it
            dQ = ops.DeviceCSR.from_scipy(Q, self._device)
            dM = ops.DeviceCSR.from_scipy(M, self._device)
            M = ops.spgemm(ops.spgemm(dQ.transpose(), dM), dQ).to_scipy()
        return out


class NeuralMG_2D(Multigrid):
    """Multigrid.py:373-765: `NeuralMG_2D(matrix, rhs, model, M, std, mean)`, the 2-D learned multigrid.
    define_hierarchy(levels) builds l_hierarchy, one transfer operator Q_l per coarsening (SciPy CSR, unit row sums), from
    the mass matrix M and the caller's model -- any object with `predict(ndarray (p, 43)) -> ndarray (p, 31)` -- on the
    device (learned_q2d.py, csrc/nmg2d.hip; the rules: DESIGN.md section 3).  The stages are callable one at a time under
    the reference's names, argument orders and result shapes, on host arrays.
    Deviations, all declared: solve() runs its cycles on l_hierarchy (the reference inherits
    Multigrid.solve, which asks the 1-D geometric interpolator and never reads l_hierarchy); fill_B returns B as CSR, not
    dense; matrices go in and out as CSR, not lil; a mass matrix the rules cannot take is refused with a ValueError
    (learned_q2d.Refused: .rule, .node) where the reference crashes late or corrupts its patches silently."""

    def __init__(self, matrix, rhs, model, M, std, mean, **kw):
        super().__init__(matrix, rhs, **kw)
        self._log("Selected 2D Neural Multigrid")
        self.label = "NeuralMG"                                              # :378
        self.model, self.M, self.std, self.mean = model, M, std, mean
        self.l_hierarchy = []
        self.setup_timings = {}            # seconds per stage of the last define_hierarchy(..., timed=True)

    # -- the stages (:400-739) ------------------------------------------------------------------
    @staticmethod
    def coarsening(M):
        """(CC, FF, CC_neighs, FF_neighs) of :401-426: the coarse and the fine nodes, both ascending, and per node the
        index array of its positive neighbours."""
        from .. import learned_q2d as L
        M = L.canonical(M)
        CC, rank = L.cf_split(M)
        rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
        off = (M.data > 0) & (M.indices != rows)
        neighs = np.split(M.indices[off].astype(np.int64), np.cumsum(np.bincount(rows[off], minlength=M.shape[0]))[:-1])
        FF = np.flatnonzero(rank < 0)
        return ([int(c) for c in CC], [int(f) for f in FF], {int(c): neighs[c] for c in CC}, {int(f): neighs[f] for f in FF})

    @staticmethod
    def map_coarse(C):
        """{coarse node: its position among the coarse nodes} (:680-684)."""
        return dict(zip((int(c) for c in C), range(len(C))))

    def _checked_mass(self, M):
        from .. import learned_q2d as L
        host = L.canonical(M)
        dM = ops.DeviceCSR.from_scipy(host, self._device)
        L.check_domain(dM)
        return host, dM

    @on_device
    def extract_patches(self, CC, M):
        """(patches (p, 43) float64, fill_idxs (p, 31) int64) of :591-677: the first patch of every coarse node at the
        node's position in CC, the second patches of the nodes with 7 neighbours after them."""
        from .. import learned_q2d as L
        host, dM = self._checked_mass(M)
        rank = L.rank_of(CC, host.shape[0])
        dCC = torch.from_numpy(np.asarray(CC, dtype=np.int32).reshape(-1)).to(self._device)
        P = L.extract_patches(dM, dCC, torch.from_numpy(rank).to(self._device))
        return P.patches.cpu().numpy(), P.fill_idx.cpu().numpy().astype(np.int64)

    @on_device
    def fill_B(self, res, idx_fill, total_size, mapping, CC):
        """(B, d_neighs) of :687-732: B (total_size x len(CC)) as SciPy CSR, and {coarse position: the coarse positions
        of its coarse second neighbours}.  `mapping` must be map_coarse(CC); the patches must be placed as
        extract_patches places them."""
        from .. import learned_q2d as L
        CC = np.asarray(CC, dtype=np.int64).reshape(-1)
        nc = CC.size
        idx = np.ascontiguousarray(np.asarray(idx_fill), dtype=np.int64).reshape(-1, 31)
        res = np.ascontiguousarray(np.asarray(res, dtype=np.float64)).reshape(-1, 31)
        rank = L.rank_of(CC, int(total_size))
        if len(mapping) != nc or any(mapping.get(int(c)) != r for r, c in enumerate(CC)):
            raise ValueError("NeuralMG_2D.fill_B: mapping is not map_coarse(CC)")
        if idx.shape[0] < nc or res.shape[0] != idx.shape[0] or not np.array_equal(idx[:nc, 0], CC) \
                or idx.min() < -1 or idx.max() >= total_size or np.any(rank[idx[nc:, 0]] < 0) \
                or np.unique(idx[nc:, 0]).size != idx.shape[0] - nc:
            raise ValueError("NeuralMG_2D.fill_B: patch j < len(CC) must belong to CC[j], each later one to a coarse node "
                             "of its own, and every index must lie in [-1, total_size)")
        last = np.arange(nc, dtype=np.int32)
        last[rank[idx[nc:, 0]]] = np.arange(nc, idx.shape[0], dtype=np.int32)
        dev = self._device
        dB, dn = L.fill_B(torch.from_numpy(res).to(dev), torch.from_numpy(idx.astype(np.int32)).to(dev),
                          torch.from_numpy(last).to(dev), torch.from_numpy(rank).to(dev), nc)
        dn = dn.cpu().numpy()
        return dB.to_scipy(), {r: dn[r][dn[r] >= 0].astype(np.int64) for r in range(nc)}

    @on_device
    def pre_process(self, mass, d_neighs):
        """The coarse mass matrix without the entries (i, j), j != i, j not in d_neighs[i] (:735-739), as SciPy CSR.
        d_neighs: fill_B's dict, or an (n, 6) integer array padded with -1."""
        from .. import learned_q2d as L
        host = L.canonical(mass)
        n = host.shape[0]
        if isinstance(d_neighs, dict):
            dn = np.full((n, 6), -1, dtype=np.int32)
            for i in range(n):
                row = np.asarray(d_neighs[i], dtype=np.int32).reshape(-1)
                if row.size > 6:
                    raise ValueError("NeuralMG_2D.pre_process: d_neighs[%d] has more than 6 entries" % i)
                dn[i, :row.size] = row
        else:
            dn = np.ascontiguousarray(np.asarray(d_neighs), dtype=np.int32)
            if dn.shape != (n, 6):
                raise ValueError("NeuralMG_2D.pre_process: d_neighs must be (%d, 6), got %s" % (n, dn.shape))
        dM = ops.DeviceCSR.from_scipy(host, self._device)
        return ops.nmg2d_cut(dM, torch.from_numpy(dn).to(self._device)).to_scipy()

    # -- :741-765 -------------------------------------------------------------------------------
    @on_device
    def define_hierarchy(self, levels=2, timed=False):
        """Sets l_hierarchy to the levels - 1 operators Q_l.  timed=True: setup_timings receives the seconds per stage."""
        from ..learned_q2d import define_hierarchy
        if levels == 1:
            self._log("Coarse grid correction not required")               # :743-744
            return
        if levels < 1:
            raise ValueError("levels must be >= 1 (levels counts grids)")
        self.setup_timings = {} if timed else self.setup_timings
        self.l_hierarchy = define_hierarchy(self.model, self.M, self.mean, self.std, levels, self._device,
                                            timings=self.setup_timings if timed else None)
        self.hierarchy = self.l_hierarchy
        self._hier = None

    def _levels(self, levels):
        if not self.l_hierarchy:
            self.define_hierarchy(2 if levels is None else levels)
        have = len(self.l_hierarchy) + 1
        if levels is not None and levels != have:
            raise ValueError("levels=%d, but the hierarchy that is defined has %d (define_hierarchy(levels) builds another)"
                             % (levels, have))
        self.hierarchy = self.l_hierarchy
        return have

    _FIRST_CALL = True

    def solve(self, levels=None, smoother="Jacobi", smooth_steps=1, max_iterations=100, error=1e-08,
              initial_guess=None, cycle="V", first_call=True, **kw):
        """The cycles of HierarchyMG(matrix, rhs, l_hierarchy) with Multigrid.solve's keywords; levels None: the levels of
        the hierarchy that is defined (define_hierarchy(2) if none is); another number: ValueError."""
        super().solve(self._levels(levels), smoother, smooth_steps, max_iterations, error, initial_guess, cycle,
                      first_call, **kw)

    def solve_many(self, rhs, levels=None, *args, **kw):
        return super().solve_many(rhs, self._levels(levels), *args, **kw)


class ClassicalAMG(Multigrid):
    """Classical AMG from the matrix alone: what the reference's scripts call as their algebraic baseline,
    `pyamg.ruge_stuben_solver(A, max_levels=2, presmoother=('gauss_seidel', {'iterations': 3}), coarse_solver='splu')`
    (test_pyAMG.py), with the setup on the device (amg.classical_hierarchy, csrc/amg.hip; the rules: DESIGN.md section 3).
    The C/F split is PMIS, not Ruge-Stueben's two sequential passes, so the levels differ from pyamg's.
    theta, split ("pmis" | "greedy"), interp_sweeps, interp_omega, interp_trunc and max_coarse as in classical_hierarchy;
    max_levels is the default of solve(levels=...), which counts grids as everywhere and is an upper limit here: the
    coarsening also stops at a level of at most max_coarse rows.  solve, v_cycle / w_cycle / f_cycle and solve_many are the
    inherited ones; level_dims reports the sizes, hierarchy_info() the setup."""

    def __init__(self, matrix, rhs, *, theta=0.25, split="pmis", interp_sweeps=1, interp_omega=1.0, interp_trunc=0.2,
                 max_coarse=500, max_levels=10, **kw):
        super().__init__(matrix, rhs, **kw)
        self._log("Selected Classical AMG")
        self.label = "ClassicalAMG"
        self.max_levels = int(max_levels)
        self._amg = dict(theta=theta, split=split, interp_sweeps=interp_sweeps, interp_omega=interp_omega,
                         interp_trunc=interp_trunc, max_coarse=max_coarse)

    _METHOD, _COUNT = "classical AMG", "n_c"          # for the "no coarse level" message

    def _build_hierarchy(self, levels, coarse_refine):
        from ..amg import classical_hierarchy
        return classical_hierarchy(sp.csr_matrix(self.matrix), self._device, max_levels=levels,
                                   coarse_refine=coarse_refine, verbose=self.verbose, **self._amg)

    def _setup_key(self):
        return tuple(sorted(self._amg.items()))

    def _setup(self, levels, first_call, coarse_refine):
        key = (levels, id(self.matrix), str(coarse_refine), self._setup_key())
        if self._hier is None or self._hier_key != key:
            H = self._build_hierarchy(levels, coarse_refine)
            if len(H.levels) < 2:
                raise ValueError("%s found no coarse level for this matrix (%d rows, max_coarse=%d, %s=%s): "
                                 "nothing to cycle on" % (self._METHOD, H.levels[0].n, self._amg["max_coarse"], self._COUNT,
                                                          H.amg_info[0][self._COUNT]))
            self._hier, self._hier_key = H, key
        return self._hier

    @on_device
    def setup(self, levels=None, coarse_refine="auto"):
        """The Hierarchy solve(levels) would run on, built now: a preconditioner= for CG and GMRES."""
        return self._setup(self.max_levels if levels is None else levels, False, coarse_refine)

    def hierarchy_info(self, levels=None):
        """{"levels": [per level n, nnz, n_c, rounds], "operator_complexity", "grid_complexity"} (amg.hierarchy_info) of the
        hierarchy in use, built first where there is none."""
        from ..amg import hierarchy_info
        return hierarchy_info(self._hier if self._hier is not None and levels is None else self.setup(levels))

    def solve(self, levels=None, *args, **kw):
        super().solve(self.max_levels if levels is None else levels, *args, **kw)

    def solve_many(self, rhs, levels=None, *args, **kw):
        return super().solve_many(rhs, self.max_levels if levels is None else levels, *args, **kw)


class SmoothedAggregationAMG(ClassicalAMG):
    """Smoothed-aggregation AMG from the matrix and one near-nullspace candidate: what a pyamg user calls as
    `pyamg.smoothed_aggregation_solver(A, B)`, with the setup on the device (aggregation.sa_hierarchy, csrc/sa.hip; the
    rules: DESIGN.md section 3).  The aggregates grow around MIS-2 roots, not by pyamg's sequential standard aggregation, and
    the Jacobi step on the tentative prolongator is scaled by the Gershgorin bound, so the levels differ from pyamg's
    (INTEGRATION.md).  theta, B (an n-vector, default ones), omega and max_coarse as in sa_hierarchy; max_levels, setup(),
    hierarchy_info(), solve, the cycle methods and solve_many as for ClassicalAMG.

    Systems: block_size = bs makes every bs consecutive unknowns one node (pyamg: the blocksize of a BSR matrix) and B may
    be an (n, k) array of k <= 6 candidates -- rigid-body modes for elasticity; rank_tol is the Cholesky pivot below which
    an aggregate whose candidates are locally dependent is refused (amg.Refused).  Both as in sa_hierarchy (csrc/nsp.hip)."""

    _METHOD, _COUNT = "smoothed aggregation", "n_agg"

    def __init__(self, matrix, rhs, *, theta=0.0, B=None, omega=4.0 / 3.0, block_size=1, rank_tol=1e-12, max_coarse=500,
                 max_levels=10, **kw):
        Multigrid.__init__(self, matrix, rhs, **kw)
        self._log("Selected Smoothed Aggregation AMG")
        self.label = "SmoothedAggregationAMG"
        self.max_levels = int(max_levels)
        self._amg = dict(theta=theta, omega=omega, block_size=block_size, rank_tol=rank_tol, max_coarse=max_coarse)
        self._candidate = B

    def _build_hierarchy(self, levels, coarse_refine):
        from ..aggregation import sa_hierarchy
        return sa_hierarchy(sp.csr_matrix(self.matrix), self._device, B=self._candidate, max_levels=levels,
                            coarse_refine=coarse_refine, verbose=self.verbose, **self._amg)

    def _setup_key(self):
        return tuple(sorted(self._amg.items())) + (id(self._candidate),)

    def hierarchy_info(self, levels=None):
        """{"levels": [per level n, nnz, n_agg, rounds], "operator_complexity", "grid_complexity"}
        (aggregation.hierarchy_info) of the hierarchy in use, built first where there is none."""
        from ..aggregation import hierarchy_info
        return hierarchy_info(self._hier if self._hier is not None and levels is None else self.setup(levels))
