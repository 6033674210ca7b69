"""Device-resident multigrid hierarchy and the V-cycle executor.

The reference rebuilds everything inside every cycle (Multigrid.py:91-106: transfer
operator lookup, `i.T @ A @ i`, SuperLU factorisation -- its own TODOs at :22-23).
Here that is the SETUP phase, done once per (matrix, transfers):
    P_l        uploaded as CSR (any scipy.sparse / ndarray input),
    R_l = P_l^T as an explicit CSR (restriction becomes a gather SpMV: deterministic,
               no atomics),
    A_{l+1} = (R_l A_l) P_l   by the device SpGEMM (lmg_spgemm_*), evaluated left to
               right like SciPy evaluates `i.T @ A @ i`,
    coarsest   A_L^-1 formed once on the device (dense, fp64) and applied per cycle by
               lmg_dense_gemv plus `coarse_refine` steps of iterative refinement
               (replaces `spsolve(A_coarse, res_coarse)` of Multigrid.py:106).
The SOLVE phase (Multigrid.py:77-124) then only launches bandwidth-bound kernels on
vectors that never leave HBM, and can be captured into a hipGraph.
"""
import math

import numpy as np
import scipy.sparse as sp
import torch

from . import ops, smoothing
from .coarse import make_coarse_solver
from .ops import DeviceCSR, F64
from .smoothing import (CHEBY_RATIO, GS_SWEEPS, LINE_DIRS, LINE_ORDERS, _directions, chebyshev_coefficients,  # noqa: F401
                        chebyshev_degree, gs_sweep_pair, line_band_value, line_config, line_half_steps)
from .twins import DiaTwin, check_values, line_reach, line_stride


CYCLE_SHAPES = ("V", "W", "F")                         # pyamg's multilevel_solver.solve(cycle=...)
KRYLOV_SHAPES = ("K",)                                 # ... and the nonlinear cycle pyamg spells cycle='AMLI' (Hierarchy.cycle)
K_INNER = ops.K_INNER                                  # the inner Krylov method of a K-cycle
_CHILDREN = {"V": ("V",), "W": ("W", "W"), "F": ("F", "V"), "K": ("K", "K")}


def cycle_children(shape):
    """The cycles a `shape` cycle runs on the next coarser level, one after the other (pyamg's convention).  A K-cycle
    runs two, each from a zero iterate, and combines them (Hierarchy._accelerated); whoever cannot do that asks
    linear_cycle_children."""
    if not isinstance(shape, str) or shape not in _CHILDREN:
        raise ValueError("cycle shape must be one of %s, got %r" % (CYCLE_SHAPES + KRYLOV_SHAPES, shape))
    return _CHILDREN[shape]


def linear_cycle_children(shape, who):
    """cycle_children for a cycle that has the linear shapes only: `who` (named in the ValueError) has no K-cycle."""
    if isinstance(shape, str) and shape in KRYLOV_SHAPES:
        raise ValueError("%s has no %r cycle: the Krylov-accelerated cycle runs on single right-hand sides of a "
                         "single-GPU Hierarchy only (Multigrid.solve, GMRES.solve); use one of %s"
                         % (who, shape, CYCLE_SHAPES))
    return cycle_children(shape)


def k_inner_name(k_inner):
    if not isinstance(k_inner, str) or k_inner not in K_INNER:
        raise ValueError("k_inner must be one of %s, got %r" % (K_INNER, k_inner))
    return k_inner


def capture_cycle(ops_mod, levels, run, swap_from=None):
    """The launches of run() captured into an ops_mod.CapturedGraph (a hipGraph), which is returned.  They hold the addresses
    of the ping-pong buffers x and tmp of `levels`, so afterwards every level must hold the tensors it held, in their
    slots.  From level swap_from on (None: nowhere) the two may have changed places: a coarse level's first visit starts
    from a zero iterate and never reads x, so a graph does not depend on where that level's iterate starts -- with
    turnaround passes (W- and F-cycles) it may end in the other buffer -- and the two are put back."""
    before = [(lev.x, lev.tmp) for lev in levels]
    g = ops_mod.CapturedGraph()
    with g:
        run()
    for l, (lev, (x, tmp)) in enumerate(zip(levels, before)):
        swapped = swap_from is not None and l >= swap_from and lev.x is tmp and lev.tmp is x
        if not swapped and (lev.x is not x or lev.tmp is not tmp):
            raise RuntimeError("ping-pong buffers did not return to their slots")
        lev.x, lev.tmp = x, tmp
    return g


# the ops predicates of the fused Chebyshev passes, by the Jacobi predicate each stands in for (Hierarchy._ask)
CHEBY_TWIN = {"stencil_smooth_available": "stencil_cheby_available",
              "stencil_smooth_prolong_available": "stencil_cheby_prolong_available",
              "stencil_smooth_restrict_available": "stencil_cheby_restrict_available"}


def _to_csr_host(M):
    """csr_matrix(...) exactly like SemiGeometricMG.__init__ (Multigrid.py:182): dense
    inputs lose their zeros, sparse inputs keep explicit zeros."""
    M = sp.csr_matrix(M, dtype=np.float64)
    if not M.has_canonical_format:
        M = M.copy()
        M.sum_duplicates()
    return M


class Level:
    __slots__ = ("n", "A", "P", "R", "x", "b", "r", "tmp", "plan_RA", "plan_RAP", "RA",
                 "gs_sched", "host_pattern", "dinv", "M", "plan_RM", "plan_RMP", "RM", "d", "line", "line_band", "kc")

    def __init__(self, A):
        self.n = A.shape[0]
        self.A = A
        self.P = self.R = None
        self.plan_RA = self.plan_RAP = self.RA = None
        dev = A.device
        self.x = torch.zeros(self.n, dtype=F64, device=dev)
        self.b = torch.zeros(self.n, dtype=F64, device=dev)
        self.r = torch.zeros(self.n, dtype=F64, device=dev)
        self.tmp = torch.zeros(self.n, dtype=F64, device=dev)
        self.gs_sched = {}
        self.host_pattern = None
        self.dinv = None
        self.d = None                  # Chebyshev smoother: the step vector of the two-launch path (prepare_smoother)
        self.line = None               # "Line" smoother: {"W": line stride, "x" / "y": factor triple} (prepare_smoother)
        self.line_band = None          # ... {"x" / "y": half-bandwidth p}; p > 1: the factors are one (2 p + 1) n block
        self.kc = None                 # K-cycle: the work vectors (rt, v1, v2, x2) of an accelerated level (_prepare_kcycle)
        self.M = None                  # mass matrix of the level (optional, see Hierarchy(mass=...))
        self.plan_RM = self.plan_RMP = self.RM = None


class Hierarchy:
    """levels[0] is the fine grid; transfers[l] (n_l x n_{l+1}) prolongates level l+1 -> l.  transfers: a list of matrices
    (anything SciPy takes, or ops.DeviceCSR with sorted, duplicate-free rows, used as they are), or a callable
    f(l, A_l) -> P or None (_each_transfer)."""

    def __init__(self, A, transfers, device, coarse_refine="auto", verbose=False, ops_mod=None,
                 use_packed=True, coarse_solver="auto", spgemm_record="lazy", mass=None, cycle_values="f64"):
        """coarse_refine: steps of iterative refinement around every coarsest-level solve; "auto" (default) measures
        the solver once at setup -- ||b - A x|| / ||b|| of one application -- and refines only when that is not at
        rounding level (the explicit block inverses of coarse.py reach 1e-14 on the Galerkin operators of grid
        problems: no refinement, half the launches and bytes of the coarsest solve).
        mass: optional fine-level mass matrix; every level then also gets M_(l+1) = Q_l^T M_l Q_l by the
        same device SpGEMM (`M_coarse = i.T @ M @ i`, Multigrid.py:273-275, and `mass = Q.T @ mass @ Q` of
        NeuralMG_2D.define_hierarchy, :763): levels[l].M, refreshed by rebuild_mass_numeric().
        cycle_values: "f64" | "f32", how the twins of every level's A, P and R store their values (H.cycle_values).  "f32":
        the cycle applies A32 = double(float(A)), P32 and R32 -- fp32 value streams in the SELL and DIA twins, vectors and
        arithmetic in fp64 -- and is a PRECONDITIONER (CG.solve / GMRES.solve(preconditioner=H)): a fixed linear operator
        close to A^-1, not a solver for A x = b (residual_norm() raises).  The Galerkin products and the coarsest
        factorisation read the fp64 CSR arrays either way.  Matrices without twins (use_packed=False, the CPU test shims)
        are not affected."""
        self.cycle_values = check_values(cycle_values, "cycle_values")
        # `ops_mod` exists for the CPU-only host-logic tests (a test shim stands in for the
        # HIP kernels); the product always runs with learnmultigrid_amd.ops.
        self.ops = ops if ops_mod is None else ops_mod
        self.device = torch.device(device)
        # every kernel wrapper launches on the CURRENT device's stream: build on the device that holds the data
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):
                self._build(A, transfers, coarse_refine, verbose, use_packed, coarse_solver, spgemm_record, mass)
        else:
            self._build(A, transfers, coarse_refine, verbose, use_packed, coarse_solver, spgemm_record, mass)

    def _build(self, A, transfers, coarse_refine, verbose, use_packed, coarse_solver, spgemm_record, mass):
        ops_ = self.ops
        self._coarse_refine_arg = coarse_refine
        self.coarse_refine = 1 if coarse_refine == "auto" else int(coarse_refine)
        self.coarse_strategy = coarse_solver
        self.verbose = verbose
        # every launch of this hierarchy goes to one explicit HIP stream (the legacy default
        # stream cannot be captured into a hipGraph)
        self.stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        A0 = A if isinstance(A, DeviceCSR) else DeviceCSR.from_scipy(A, self.device)
        self.levels = [Level(A0)]
        if mass is not None:
            self.levels[0].M = mass if isinstance(mass, DeviceCSR) else DeviceCSR.from_scipy(_to_csr_host(mass), self.device)
            if self.levels[0].M.shape != A0.shape:
                raise ValueError("mass matrix %s does not match the operator %s" % (self.levels[0].M.shape, A0.shape))
        for P in self._each_transfer(transfers):
            lev = self.levels[-1]
            # a DeviceCSR (sorted, duplicate-free rows) is used as it is: no host copy
            Ph = P if isinstance(P, DeviceCSR) else _to_csr_host(P)
            if Ph.shape[0] != lev.n:
                raise ValueError("transfer operator of level %d has %d rows, level has %d unknowns"
                                 % (len(self.levels) - 1, Ph.shape[0], lev.n))
            lev.P = Ph if isinstance(P, DeviceCSR) else DeviceCSR.from_scipy(Ph, self.device)
            lev.R = lev.P.transpose()
            lev.plan_RA = ops_.SpGEMMPlan(lev.R, lev.A, spgemm_record)
            lev.RA = lev.plan_RA.numeric(lev.R, lev.A)
            lev.plan_RAP = ops_.SpGEMMPlan(lev.RA, lev.P, spgemm_record)
            Ac = lev.plan_RAP.numeric(lev.RA, lev.P)
            self.levels.append(Level(Ac))
            if lev.M is not None:
                lev.plan_RM = ops_.SpGEMMPlan(lev.R, lev.M, spgemm_record)
                lev.RM = lev.plan_RM.numeric(lev.R, lev.M)
                lev.plan_RMP = ops_.SpGEMMPlan(lev.RM, lev.P, spgemm_record)
                self.levels[-1].M = lev.plan_RMP.numeric(lev.RM, lev.P)
        self.use_packed = bool(use_packed)
        self._pack_all()
        self._inverse_diagonals()
        self.partials = torch.empty(ops_.partials_count(self.levels[0].n), dtype=F64, device=self.device)
        self.outer_r = torch.zeros(self.levels[0].n, dtype=F64, device=self.device)
        self.norm2 = torch.zeros(1, dtype=F64, device=self.device)
        self._factor_coarsest()
        self.generation = 0            # counts rebuild_numeric(): holders of state derived from the values compare it (block.py)
        self._graphs = {}
        self._cheby = None             # Chebyshev smoother: bounds and coefficient tables (prepare_smoother)
        self._line = None              # "Line" smoother: the (line_dir, line_order) in use (prepare_smoother)
        self._line_band = 1            # ... and the largest half-bandwidth a level may use (line_band)
        self.kscal = self.kpartials = None   # K-cycle: the scalars of every accelerated level, the scratch of the steps

    def _each_transfer(self, transfers):
        """The transfers one by one.  A callable f(l, A_l) -> P or None is asked once per level with that level's DeviceCSR,
        after the level was formed (a setup that builds P from A_l: amg.classical_hierarchy); None ends the coarsening."""
        if not callable(transfers):
            yield from transfers
            return
        while True:
            P = transfers(len(self.levels) - 1, self.levels[-1].A)
            if P is None:
                return
            yield P

    # ------------------------------------------------------------------ setup ----------
    @property
    def sizes(self):
        return [lev.n for lev in self.levels]

    def _pack_all(self):
        """Packed twins (lossless, fewer HBM bytes) of every operator the sweeps touch."""
        if not self.use_packed:
            return
        for lev in self.levels:
            for M in (lev.A, lev.P, lev.R):
                if M is not None and hasattr(M, "pack"):
                    M.pack(values=self.cycle_values)

    def _cycle_source(self, A):
        """The matrix the sweeps on A apply, as plain CSR: A itself, or -- twins that hold fp32 values -- its rounded view
        (DeviceCSR.cycle_source), so that what the host derives for a smoother agrees with what the kernels load."""
        return A.cycle_source() if getattr(A, "twin_values", "f64") == "f32" else A

    def _inverse_diagonal(self, lev):
        return self.ops.csr_inverse_diagonal(self._cycle_source(lev.A))

    def _inverse_diagonals(self):
        # for the zero-initial-guess first sweep on coarse levels (allocated at setup so that
        # nothing has to be allocated while a hipGraph is being captured)
        for lev in self.levels[1:-1]:
            lev.dinv = self._inverse_diagonal(lev)

    def _factor_coarsest(self):
        """Direct solver of the coarsest operator (setup): dense inverse, or the banded block
        elimination of coarse.py when the operator is narrow-banded (grid problems)."""
        A = self.levels[-1].A
        old = getattr(self, "coarse", None)
        if old is not None and hasattr(old, "factor") and old.n == A.shape[0]:
            try:
                old.factor(A)                          # same pattern: numeric phase only
                self._measure_coarse()
                return
            except ValueError:
                pass
        self.coarse = make_coarse_solver(A, self.ops, self.coarse_strategy)
        self._measure_coarse()

    COARSE_AUTO_TOL = 1e-12

    def _measure_coarse(self):
        """coarse_refine="auto": one application of the fresh factors on a fixed right-hand side; its relative residual
        decides whether the cycles refine (setup only: one SpMV, one solve, two 8-byte reads)."""
        if self._coarse_refine_arg != "auto":
            return
        lev = self.levels[-1]
        n = lev.n
        g = torch.Generator().manual_seed(1234)
        bh = torch.rand(n, dtype=F64, generator=g) - 0.5
        nb = float(bh.norm())
        b = bh.to(self.device)
        x = torch.zeros(n, dtype=F64, device=self.device)
        self.coarse.apply(b, x)
        # (own kernels only: no library load.  What is measured is the factorisation, which reads the fp64 values: with
        # fp32 twins the residual is taken on the plain CSR arrays, not on A32)
        A = lev.A.plain() if getattr(lev.A, "twin_values", "f64") == "f32" else lev.A
        self.ops.csr_residual_norm2(A, x, b, None, self.partials, self.norm2)
        rel = math.sqrt(max(float(self.norm2.item()), 0.0)) / nb
        self.coarse_residual = rel
        self.coarse_refine = 0 if rel <= self.COARSE_AUTO_TOL else 1

    def rebuild_numeric(self, new_vals):
        """Galerkin rebuild after the VALUES of the fine matrix changed (same pattern):
        numeric SpGEMM passes only, then the coarse factorisation (config #5)."""
        if self.device.type == "cuda" and torch.cuda.current_device() != self.device.index and self.device.index is not None:
            with torch.cuda.device(self.device):
                return self.rebuild_numeric(new_vals)
        A0 = self.levels[0].A
        if new_vals.numel() != A0.nnz:
            raise ValueError("rebuild_numeric needs the same sparsity pattern")
        A0.vals.copy_(new_vals)
        for l in range(len(self.levels) - 1):
            lev = self.levels[l]
            lev.plan_RA.numeric(lev.R, lev.A, out=lev.RA)
            lev.plan_RAP.numeric(lev.RA, lev.P, out=self.levels[l + 1].A)
        if self.use_packed:
            for lev in self.levels:
                lev.A.repack_values()            # same pattern: only the value streams change
        for lev in self.levels:
            for sched in lev.gs_sched.values():
                # the one schedule that holds values: its twin follows them (the backward schedule shares the forward one's)
                if sched.kind == "multicolor_device" and not sched.backward:
                    self._ask("gs_refresh", lev.A, sched)
        self._inverse_diagonals()
        if self.levels[0].dinv is not None:          # (made on first use by a smoother that needs it: follows the values too)
            self.levels[0].dinv = self._inverse_diagonal(self.levels[0])
        self._factor_coarsest()
        self.generation += 1                         # (after the factorisation: H.coarse may be a solver of another kind now)
        self._graphs = {}
        for smoother in smoothing.STATEFUL:          # new values: new bounds and tables, new factors
            self._prepare(smoother, renew=True)

    # ------------------------------------------------------------------ line relaxation --
    OFFSET_CHUNK_ROWS = 1 << 16        # rows per step of _device_offsets

    def _device_offsets(self, l):
        """The distinct values of column - row of level l, ascending, found on the device in chunks of OFFSET_CHUNK_ROWS
        rows: no host copy of the pattern and a transient of one chunk's entries.  The chunk boundaries of rowptr come to
        the host in one read; every chunk then costs the synchronisations of two torch.unique calls and a size read, and
        the result (at most 49 values) one more read.  Stops with None once there are more than 49 values (no 7x7 window
        holds them)."""
        A = self.levels[l].A
        n = A.shape[0]
        cuts = list(range(0, n, self.OFFSET_CHUNK_ROWS)) + [n]
        ends = A.rowptr[torch.tensor(cuts, dtype=torch.int64, device=A.rowptr.device)].cpu().tolist()
        seen = None
        for (r0, r1), (e0, e1) in zip(zip(cuts[:-1], cuts[1:]), zip(ends[:-1], ends[1:])):
            counts = (A.rowptr[r0 + 1:r1 + 1] - A.rowptr[r0:r1]).to(torch.int64)
            rows = torch.repeat_interleave(torch.arange(r0, r1, dtype=torch.int64, device=counts.device), counts,
                                           output_size=e1 - e0)
            u = torch.unique(A.colidx[e0:e1].to(torch.int64) - rows)
            seen = u if seen is None else torch.unique(torch.cat((seen, u)))
            if seen.numel() > 49:
                return None
        return np.zeros(0, dtype=np.int64) if seen is None else seen.cpu().numpy()

    def _line_stride(self, l, radius=1):
        """(W, reach): the line stride of level l and the half-bandwidths (x, y) its line systems need -- those of its grid
        twin (3x3: (1, 1)), or the stride its offsets fit with the smallest window radius <= `radius` (twins.line_stride):
        on the host for small levels, whose twins are never built, and for radius > 1 from the offsets the device lists
        for the larger ones (_device_offsets).  (None, None): no such geometry."""
        lev = self.levels[l]
        for twin in (getattr(lev.A, "stencil", None), getattr(lev.A, "dia", None)):
            if twin is not None:
                return int(twin.W), (1, 1)
        if lev.n >= DiaTwin.MIN_ROWS:
            off = self._device_offsets(l) if radius > 1 else None
        else:
            if lev.host_pattern is None:
                lev.host_pattern = (lev.A.rowptr.cpu().numpy(), lev.A.colidx.cpu().numpy())
            rp, ci = lev.host_pattern
            rows = np.repeat(np.arange(lev.n, dtype=np.int64), np.diff(rp))
            off = np.unique(ci.astype(np.int64) - rows)
        if off is None:
            return None, None
        for rad in range(1, radius + 1):
            W = line_stride(off, lev.n, rad)
            if W is not None:
                return int(W), line_reach(off, int(W), rad)
        return None, None

    def _line_geometry(self, l, band):
        """(W, {"x": p, "y": p}) of level l under the largest half-bandwidth `band`, or the ValueError that names the level
        and why it cannot run the Line smoother."""
        lev = self.levels[l]
        W, reach = self._line_stride(l, band)
        if W is None:
            raise ValueError("the Line smoother cannot run on level %d (%d rows): no %dx%d grid geometry"
                             % (l, lev.n, 2 * band + 1, 2 * band + 1))
        if lev.n % W != 0:
            raise ValueError("the Line smoother cannot run on level %d: its %d rows are no whole lines of %d "
                             "(n %% W != 0)" % (l, lev.n, W))
        if W == lev.n:
            raise ValueError("the Line smoother cannot run on level %d: one line of %d rows (W == n, a 1-D operator)"
                             % (l, lev.n))
        return W, {"x": reach[0], "y": reach[1]}

    def _factor_lines(self, dirs):
        """The factors of every smoothed level for the directions `dirs` that it does not have yet (one flag read each)."""
        for l, lev in enumerate(self.levels[:-1]):
            if lev.line is None:
                W, lev.line_band = self._line_geometry(l, self._line_band)
                lev.line = {"W": W}
            for d in dirs:
                if d not in lev.line:
                    factor, _ = smoothing.line_ops(self.ops, lev.line_band[d])
                    try:
                        lev.line[d] = factor(lev.A, lev.line["W"], d)
                    except ValueError as e:
                        raise ValueError("the Line smoother cannot run on level %d (%d rows, line stride %d): %s"
                                         % (l, lev.n, lev.line["W"], e)) from None

    def _discard_lines(self, levels):
        """Forget the line factors of `levels`.  A captured Line cycle holds their addresses, not the tensors: every
        captured Line cycle goes with them."""
        for lev in levels:
            lev.line = lev.line_band = None
        self._graphs = {k: g for k, g in self._graphs.items() if k[0] != "Line"}

    def _use_line_band(self, band):
        """Make `band` the largest half-bandwidth in use.  A level the new window refuses raises before anything changes:
        the band in use, its factors and the captured cycles stay.  A level whose stride and half-bandwidths are the same
        under both windows keeps its factors (a 3x3 level always does); only a level that reads differently is
        factored anew."""
        smoothed = self.levels[:-1]
        geometry = [self._line_geometry(l, band) for l in range(len(smoothed))]
        stale = [lev for lev, (W, p) in zip(smoothed, geometry) if lev.line is not None and (lev.line["W"], lev.line_band) != (W, p)]
        if stale:
            self._discard_lines(stale)
        for lev, (W, p) in zip(smoothed, geometry):
            if lev.line is None:
                lev.line, lev.line_band = {"W": W}, p
        self._line_band = band

    def _prepare_line(self, line_dir=None, line_order=None, line_band=None, renew=False):
        """All None: keep what is prepared (the defaults when nothing is).  line_band None: the band in use (1 at first).
        renew: the values have changed -- new factors for every direction that had them (none where nothing is prepared)."""
        if renew:
            if self._line is not None:
                had = sorted({d for lev in self.levels[:-1] for d in (lev.line or ()) if d != "W"})
                for lev in self.levels[:-1]:
                    lev.line = lev.line_band = None
                for d in had:
                    self._factor_lines(d)
            return
        band = line_band_value(line_band)
        keep = self._line is not None and line_dir is None and line_order is None
        if keep and band in (None, self._line_band):
            return
        cfg = self._line if keep else line_config(line_dir, line_order)
        if band not in (None, self._line_band):
            self._use_line_band(band)
            self._line = None
            try:
                self._factor_lines(cfg[0])
            except ValueError:                       # (a pivot, a coupled line: nothing is prepared, back to the default)
                self._discard_lines(self.levels[:-1])
                self._line_band = 1
                raise
        else:
            self._factor_lines(cfg[0])
        self._line = cfg

    def line_key(self):
        """What a captured Line cycle depends on besides the cycle's own arguments: (line_dir, line_order) in use, and the
        largest half-bandwidth line_band where it is not 1."""
        return self._line if self._line is None or self._line_band == 1 else self._line + (self._line_band,)

    # ------------------------------------------------------------------ Chebyshev ------
    def _prepare_chebyshev(self, cheby_lmax=None, cheby_ratio=None, renew=False):
        """Bounds [lmax / ratio, lmax] of D^-1 A on every smoothed level, the inverse diagonals and the step vectors of
        the two-launch path.  cheby_lmax: None = the Gershgorin bound of each level (one small launch and one 8-byte
        read per level), a float for all levels, or one value per smoothed level.  Both None: keep what is prepared.
        renew: the values have changed -- new bounds and tables from the arguments in use, nothing where none were prepared."""
        if renew:
            if self._cheby is None:
                return
            (cheby_lmax, cheby_ratio), self._cheby = self._cheby["args"], None
        if self._cheby is not None and cheby_lmax is None and cheby_ratio is None:
            return
        ratio = CHEBY_RATIO if cheby_ratio is None else float(cheby_ratio)
        chebyshev_coefficients(1.0, ratio, 1)                     # (checks the ratio)
        nl = len(self.levels) - 1
        if cheby_lmax is None or isinstance(cheby_lmax, (int, float)):
            given = [cheby_lmax] * nl
        else:
            given = list(cheby_lmax)
            if len(given) != nl:
                raise ValueError("cheby_lmax needs one value per smoothed level (%d), got %d" % (nl, len(given)))
        args = (None if cheby_lmax is None else tuple(float(v) for v in given), ratio)
        if self._cheby is not None and self._cheby["args"] == args:
            return
        lmax = []
        for lev, g in zip(self.levels[:-1], given):
            if g is None:
                self.ops.csr_gershgorin(self._cycle_source(lev.A), self.norm2)
                g = float(self.norm2.item())
            chebyshev_coefficients(g, ratio, 1)                   # (checks the bound)
            lmax.append(float(g))
            if lev.dinv is None:
                lev.dinv = self._inverse_diagonal(lev)
            if lev.d is None:
                lev.d = torch.zeros(lev.n, dtype=F64, device=self.device)
        self._cheby = {"args": args, "lmax": lmax, "ratio": ratio, "coef": {}}

    def cheby_key(self):
        """What a captured Chebyshev cycle depends on besides the cycle's own arguments: the bounds in use."""
        return None if self._cheby is None else (tuple(self._cheby["lmax"]), self._cheby["ratio"])

    def _cheby_coef(self, l, degree):
        ch = self._cheby
        if ch is None:
            raise RuntimeError("Chebyshev smoother used before prepare_smoother")
        key = (l, degree)
        if key not in ch["coef"]:
            ch["coef"][key] = chebyshev_coefficients(ch["lmax"][l], ch["ratio"], degree)
        return ch["coef"][key]

    def _prepare(self, smoother, cheby_lmax=None, cheby_ratio=None, line_dir=None, line_order=None, line_band=None, renew=False):
        """Bring the state of `smoother` to what its own keywords of prepare_smoother ask for (renew: to the new values of the
        matrices); those of another smoother are not looked at.  The one place that knows which smoothers keep state here."""
        if smoother == "Chebyshev":
            self._prepare_chebyshev(cheby_lmax, cheby_ratio, renew)
        elif smoother == "Line":
            self._prepare_line(line_dir, line_order, line_band, renew)

    def _smoother_key(self, smoother):
        """What a captured cycle of `smoother` depends on besides the cycle's own arguments, as the tail of its key."""
        return {"Chebyshev": (self.cheby_key(),), "Line": (self.line_key(),)}.get(smoother, ())

    def rebuild_mass_numeric(self, new_vals):
        """New values of the fine mass matrix on the same pattern: numeric SpGEMM passes only."""
        M0 = self.levels[0].M
        if M0 is None or new_vals.numel() != M0.nnz:
            raise ValueError("rebuild_mass_numeric needs a hierarchy built with mass= and the same sparsity pattern")
        M0.vals.copy_(new_vals)
        for l in range(len(self.levels) - 1):
            lev = self.levels[l]
            lev.plan_RM.numeric(lev.R, lev.M, out=lev.RM)
            lev.plan_RMP.numeric(lev.RM, lev.P, out=self.levels[l + 1].M)

    def gs_schedule(self, l, kind, direction="forward"):
        """Schedule of the Gauss-Seidel sweep on level l, cached per (kind, direction): a backward sweep runs the sets of
        the forward schedule in reverse order (GSSchedule.reversed), with its own schedule-ordered pattern copy."""
        lev = self.levels[l]
        key = kind if direction == "forward" else (kind, direction)
        if key not in lev.gs_sched:
            # built and prepared HERE, eagerly (captured_cycle only calls gs_schedule before the capture)
            if direction == "backward":
                lev.gs_sched[key] = self.gs_schedule(l, kind).reversed()
                self._ask("gs_prepare", lev.A, lev.gs_sched[key])
            elif direction != "forward":
                raise ValueError("unknown Gauss-Seidel sweep direction %r" % (direction,))
            elif kind == "multicolor_device":
                # coloured, ordered and re-encoded on the device (one colouring per level: the backward schedule above
                # shares its twin); the pattern never comes to the host
                sched = self._ask("build_gs_schedule_device", lev.A)
                if sched is False:
                    raise ValueError("gs_mode 'multicolor_device' needs an ops module with build_gs_schedule_device")
                lev.gs_sched[key] = sched
            else:
                if lev.host_pattern is None:
                    lev.host_pattern = (lev.A.rowptr.cpu().numpy(), lev.A.colidx.cpu().numpy())
                lev.gs_sched[key] = smoothing.gs_schedule(self.ops, lev.A, *lev.host_pattern, kind, self.device)
        return lev.gs_sched[key]

    # ------------------------------------------------------------------ solve ----------
    def smooth(self, l, smoother, steps, omega, gs_mode, x_is_zero=False, direction="forward"):
        """`steps` smoothing sweeps on level l.  x_is_zero: the iterate is known to be zero
        (coarse levels start from zeros, Multigrid.py:103): the first Jacobi sweep then is
        x = omega * (D^-1 b) -- same bits, a third of the bytes -- and nobody has to clear x.
        direction (Gauss-Seidel only): "forward" | "backward" | "symmetric" (pyamg's sweep: a forward then a backward
        sweep per step -- two launches per step, the backward sweep cannot start before the forward one has finished)."""
        lev = self.levels[l]
        if steps <= 0:
            if x_is_zero:
                self.ops.zero(lev.x)
            return
        if smoother == "GaussSeidel":
            if x_is_zero:
                self.ops.zero(lev.x)
            if direction == "symmetric":
                for _ in range(steps):
                    self._gs(l, gs_mode, 1, "forward")
                    self._gs(l, gs_mode, 1, "backward")
            else:
                self._gs(l, gs_mode, steps, direction)
        elif smoother == "Jacobi":
            if x_is_zero:
                if lev.dinv is None:
                    lev.dinv = self._inverse_diagonal(lev)
                self.ops.vmul(omega, lev.dinv, lev.b, lev.tmp)
                lev.x, lev.tmp = lev.tmp, lev.x
                steps -= 1
            for _ in range(steps):
                self.ops.csr_jacobi(lev.A, lev.x, lev.b, omega, lev.tmp)
                lev.x, lev.tmp = lev.tmp, lev.x
        elif smoother == "Chebyshev":
            smoothing.chebyshev_step(self.ops, lev.A, lev, self._cheby_coef(l, steps), x_is_zero)
        elif smoother == "Line":
            # per half-step: r = b - A x, then x += omega T^-1 r on its systems, in place (direction "backward": the
            # post-smoothing half, directions and colours reversed)
            if self._line is None or lev.line is None:
                raise RuntimeError("Line smoother used before prepare_smoother")
            if direction not in ("forward", "backward"):
                raise ValueError("the Line smoother runs 'forward' (pre-smoothing) or 'backward' (post-smoothing), got %r"
                                 % (direction,))
            if x_is_zero:
                self.ops.zero(lev.x)
            for _ in range(steps):
                for d, first, step in line_half_steps(*self._line, reverse=(direction == "backward")):
                    if x_is_zero:
                        self.ops.copy(lev.b, lev.r)                                  # b - A 0 = b
                        x_is_zero = False
                    else:
                        self.ops.csr_residual_norm2(lev.A, lev.x, lev.b, lev.r, None, None)
                    _, solve = smoothing.line_ops(self.ops, lev.line_band[d])
                    solve(lev.line["W"], d, first, step, lev.line[d], lev.r, omega, lev.x)
        else:
            raise ValueError("unknown smoother %r" % (smoother,))

    def _gs(self, l, gs_mode, steps, direction):
        lev = self.levels[l]
        smoothing.gauss_seidel(self.ops, lev.A, lev, self._wavefront_gs(l, gs_mode, direction),
                               lambda: self.gs_schedule(l, gs_mode, direction), steps, direction)

    def _ask(self, name, *args, smoother=None):
        """self.ops.<name>(*args), or False where the ops module has no such name (an ops module leaves out what it does
        not offer).  With smoother "Chebyshev", the Chebyshev twin of a Jacobi predicate is asked in its place."""
        if smoother == "Chebyshev":
            name = CHEBY_TWIN[name]
        return smoothing.ask(self.ops, name, *args)

    def _wavefront_gs(self, l, gs_mode, direction="forward"):
        return gs_mode == "lexicographic" and smoothing.wavefront_gs(self.ops, self.levels[l].A, direction)

    def _fusable(self, l, smoother, steps):
        if smoother not in ("Jacobi", "Chebyshev") or steps < 1:
            return False
        if not self._ask("stencil_smooth_available", self.levels[l].A, smoother=smoother):
            return False
        # a Chebyshev step is one pass: d is never carried between launches
        return smoother == "Jacobi" or steps <= self.ops.FUSED_MAX_SWEEPS

    def smooth_fused(self, l, steps, omega, x_is_zero=False, want_residual=False, correction=None, restrict_to=None,
                     smoother="Jacobi"):
        """`steps` Jacobi sweeps on level l (and r = b - A x afterwards) as fused passes of at most
        FUSED_MAX_SWEEPS sweeps each (lmg_stencil_smooth): same bits as smooth() + the residual launch,
        a third of the passes over the level's vectors.  correction = (P, e): the first pass starts from
        x + P e (Multigrid.py:115 folded in; the caller has checked stencil_smooth_prolong_available).
        smoother "Chebyshev": one step of degree `steps` (<= FUSED_MAX_SWEEPS, see _fusable) as the one pass, with its
        coefficient table in place of (omega, sweeps)."""
        coef = self._cheby_coef(l, steps) if smoother == "Chebyshev" and steps > 0 else None
        smoothing.fused_passes(self.ops, self.levels[l].A, self.levels[l], steps, omega, x_is_zero, want_residual,
                               correction, restrict_to, coef)

    def coarse_solve(self):
        lev = self.levels[-1]
        self.coarse.apply(lev.b, lev.x)
        for _ in range(self.coarse_refine):
            self.ops.csr_residual_norm2(lev.A, lev.x, lev.b, lev.r, None, None)
            if getattr(self.coarse, "supports_accumulate", False):
                self.coarse.apply(lev.r, lev.x, accumulate=True)      # x += A^-1 r in the solver's last launch
            else:
                self.coarse.apply(lev.r, lev.tmp)
                self.ops.axpby(1.0, lev.tmp, 1.0, lev.x)

    # ------------------------------------------------------------------ K-cycle --------
    def _prepare_kcycle(self):
        """What a K-cycle needs beyond the other shapes, made once (never inside a capture: cycle() and captured_cycle() come
        here first): four work vectors on every accelerated level -- the levels 1 .. L-1, whose visits the level above
        combines --, nine scalars for each of them in one buffer, and the scratch of the two steps."""
        missing = [name for name in ("kcycle_step1", "kcycle_step2") if not hasattr(self.ops, name)]
        if missing:
            raise ValueError("cycle shape 'K' needs an ops module with kcycle_step1 and kcycle_step2; this one (%s) lacks %s"
                             % (getattr(self.ops, "__name__", type(self.ops).__name__), " and ".join(missing)))
        inner = self.levels[1:-1]
        if self.kscal is not None or not inner:
            return
        for lev in inner:
            lev.kc = tuple(torch.zeros(lev.n, dtype=F64, device=self.device) for _ in range(4))
        ns = len(ops.KCYCLE_SCALARS)
        scal = torch.zeros(ns * len(inner), dtype=F64, device=self.device)
        self.kscal = [None] + [scal[ns * i:ns * (i + 1)] for i in range(len(inner))]
        count = self._ask("kcycle_partials_count", inner[0].n)           # (the largest accelerated level)
        self.kpartials = torch.zeros(max(int(count), 1), dtype=F64, device=self.device)

    def _accelerated(self, smoother, steps, omega, gs_mode, l, last, pair, k_inner):
        """The coarse correction of a K-cycle on level l < last: levels[l].b holds the right-hand side b_c, levels[l].x
        receives two steps of flexible GCR or CG on A_l x = b_c from zero, preconditioned by one K-cycle visit of level l
        (cycle()).  Per call: the two visits, two products with A_l, one launch sequence each of ops.kcycle_step1 and
        kcycle_step2; the coefficients never leave the device.  The second visit runs on other buffers -- its right-hand
        side is rt where step 1 wrote it, its iterate and scratch are the level's spare buffer and a work vector -- so b_c, c1
        and v1 stay as they are; afterwards b is back in its slot and x and tmp hold the level's own two buffers."""
        lev = self.levels[l]
        rt, v1, v2, x2 = lev.kc
        scal = self.kscal[l]

        def visit():
            self._visit(smoother, steps, omega, gs_mode, l, last, cycle_children("K"), pair, x_is_zero=True, k_inner=k_inner)

        visit()
        b, c1, spare = lev.b, lev.x, lev.tmp
        self.ops.csr_spmv(lev.A, c1, v1, 1.0, 0.0)
        self.ops.kcycle_step1(k_inner, c1, v1, b, rt, scal, self.kpartials)
        lev.b, lev.x = rt, x2
        try:
            visit()
            c2 = lev.x                                                    # (the spare buffer or x2)
            self.ops.csr_spmv(lev.A, c2, v2, 1.0, 0.0)
            self.ops.kcycle_step2(k_inner, c1, v1, c2, v2, rt, scal, spare, self.kpartials)
        finally:
            lev.b, lev.x, lev.tmp = b, spare, c1

    def cycle(self, smoother, steps, omega=1.0, gs_mode="lexicographic", l=0, depth=None,
              after_presmooth=None, x_is_zero=False, gs_sweep=("forward", "forward"), shape="V", *,
              cheby_lmax=None, cheby_ratio=None, line_dir=None, line_order=None, line_band=None, k_inner="gcr"):
        """One V(steps, steps) cycle on level l: levels[l].x is the iterate, levels[l].b the
        right-hand side (Multigrid.py:77-124).  depth = number of grids used.
        gs_sweep: directions of the Gauss-Seidel pre- and post-smoothing, a pyamg sweep name for both or a (pre, post)
        pair.  ("forward", "backward") with R = P^T, Galerkin coarse operators and the direct coarse solve makes the
        cycle a symmetric operator (a CG preconditioner); each half is one pipelined launch of the wavefront kernel,
        while a "symmetric" step costs a launch per direction.
        shape: "V" | "W" | "F" (pyamg's cycle=, CYCLE_SHAPES): what follows the restriction on every level above the
        second-coarsest -- one V-cycle, two W-cycles, or an F-cycle then a V-cycle on the next level, the second visit
        starting from the first one's iterate with the same right-hand side; the coarsest level is solved once per
        visit of the level above it.  Where a level runs the tiled Jacobi passes, the post-smoothing of one visit and
        the pre-smoothing of the next run as one turnaround pass (ops.stencil_smooth_turnaround).
        shape "K" (KRYLOV_SHAPES; Notay and Vassilevski's K-cycle, pyamg's cycle='AMLI'): on every level below the finest
        but the coarsest, the coarse system A x_c = b_c is solved by two steps of a flexible Krylov method preconditioned by
        the K-cycle of that level, each visit from a zero iterate (pyamg starts from ones):
            c1 = visit(b_c), v1 = A c1, p1 = v1 ("gcr") | c1 ("fcg"), t1 = <p1, b_c> / <p1, v1>, rt = b_c - t1 v1,
            c2 = visit(rt),  v2 = A c2, p2 likewise, gamma = <p2, v1>, beta = <p2, v2>, alpha2 = <p2, rt>, q = gamma / rho1,
            rho2 = beta - gamma q, t2 = alpha2 / rho2, x_c = (t1 - q t2) c1 + t2 c2      (a quotient by 0 is 0)
        with the products, coefficients and updates in ops.kcycle_step1 / kcycle_step2 on the device: always two steps, no
        early exit, the launch sequence is fixed (captured_cycle) and the work is a W-cycle's plus two products with A per
        visit.  The cycle is a nonlinear operator: a preconditioner for flexible methods (GMRES.solve), not for CG.
        k_inner "gcr" (default) minimises the residual and takes any operator; "fcg" is for symmetric positive definite
        operators with symmetric cycles.  A two-level hierarchy runs the V-cycle, bit for bit.  No turnaround passes.
        smoother "Chebyshev": `steps` is the DEGREE of the one polynomial smoothing step run before and after the coarse
        correction, on [lmax / cheby_ratio, lmax] of D^-1 A per level (omega is not used).  cheby_lmax / cheby_ratio as in
        prepare_smoother; left None they are what was prepared (the Gershgorin bounds and CHEBY_RATIO by default).
        smoother "Line": `steps` line relaxation steps with damping omega on either side -- line_dir "x" | "y" | "xy",
        line_order "zebra" | "jacobi" as in prepare_smoother, left None what was prepared ("xy", "zebra" by default); the
        post-smoothing half runs the directions and colours in reverse (gs_sweep is not used).  line_band as in
        prepare_smoother, left None the band in use."""
        children = cycle_children(shape)
        k_inner = k_inner_name(k_inner) if shape in KRYLOV_SHAPES else None
        if smoother == "Chebyshev":
            chebyshev_degree(steps)
        pair = gs_sweep_pair(gs_sweep)
        self._prepare(smoother, cheby_lmax, cheby_ratio, line_dir, line_order, line_band)
        if k_inner is not None:
            self._prepare_kcycle()
        if smoother == "Line":
            pair = ("forward", "backward")
        self._visit(smoother, steps, omega, gs_mode, l, (len(self.levels) if depth is None else depth) - 1, children,
                    pair, x_is_zero, after_presmooth, k_inner=k_inner)

    def _visit(self, smoother, steps, omega, gs_mode, l, last, children, pair, x_is_zero=False, after_presmooth=None,
               entered=False, leave_open=False, k_inner=None):
        """One cycle on level l whose recursion below is `children` (cycle_children of its shape).  entered: the
        pre-smoothing and the restriction have run already (in a turnaround pass).  leave_open: a visit of the same level
        follows -- return True without the post-smoothing where a turnaround pass can run it together with that visit's
        pre-smoothing.  k_inner: a K-cycle -- the two visits of the next level are combined by _accelerated."""
        if not entered:
            self._presmooth(smoother, steps, omega, gs_mode, l, x_is_zero, pair[0], after_presmooth)
        if l + 1 == last:
            self.coarse_solve()                                               # :106
        elif k_inner is not None:
            self._accelerated(smoother, steps, omega, gs_mode, l + 1, last, pair, k_inner)
        else:
            open_ = False
            for i, sub in enumerate(children):
                more = i + 1 < len(children)
                if open_:
                    self._turnaround(l + 1, steps, omega)
                open_ = self._visit(smoother, steps, omega, gs_mode, l + 1, last, cycle_children(sub), pair,
                                    x_is_zero=(i == 0), entered=open_, leave_open=more)     # zeros, :103
        if leave_open and self._turnaround_ok(l, smoother, steps):
            return True
        self._postsmooth(smoother, steps, omega, gs_mode, l, pair[1])
        return False

    def _presmooth(self, smoother, steps, omega, gs_mode, l, x_is_zero, pre, after_presmooth):
        """Pre-smoothing of level l, residual, b_(l+1) = R r (Multigrid.py:88-93)."""
        lev, nxt = self.levels[l], self.levels[l + 1]
        fused = self._fusable(l, smoother, steps)
        restricted = fused and self._ask("stencil_smooth_restrict_available", lev.A, lev.R, smoother=smoother)
        if restricted:
            self.smooth_fused(l, steps, omega, x_is_zero, restrict_to=(lev.R, nxt.b), smoother=smoother)   # :88 + :90 + :93 in one pass
        elif fused:
            self.smooth_fused(l, steps, omega, x_is_zero, want_residual=True, smoother=smoother)  # :88 + :90 in one pass
        else:
            self.smooth(l, smoother, steps, omega, gs_mode, x_is_zero, pre)       # :88
        if after_presmooth is not None:
            after_presmooth(lev.x)
        if not fused:
            self.ops.csr_residual_norm2(lev.A, lev.x, lev.b, lev.r, None, None)        # :90
        if not restricted:
            self.ops.csr_spmv(lev.R, lev.r, nxt.b, 1.0, 0.0)                       # :93

    def _postsmooth(self, smoother, steps, omega, gs_mode, l, post):
        """x += P x_(l+1), post-smoothing of level l (Multigrid.py:115-121)."""
        lev, nxt = self.levels[l], self.levels[l + 1]
        fused = self._fusable(l, smoother, steps)
        if fused and self._ask("stencil_smooth_prolong_available", lev.A, lev.P, smoother=smoother):
            self.smooth_fused(l, steps, omega, correction=(lev.P, nxt.x), smoother=smoother)     # :115 + :121 in one pass
            return
        self.ops.csr_spmv(lev.P, nxt.x, lev.x, 1.0, 1.0)                           # :115
        if fused:
            self.smooth_fused(l, steps, omega, smoother=smoother)             # :121
        else:
            self.smooth(l, smoother, steps, omega, gs_mode, direction=post)       # :121

    def _turnaround_ok(self, l, smoother, steps):
        lev = self.levels[l]
        # (Jacobi only: the Chebyshev step has no turnaround pass -- its post- and pre-passes stay separate)
        return bool(smoother == "Jacobi" and self._fusable(l, smoother, steps)
                    and self._ask("stencil_smooth_turnaround_selected", lev.A, lev.P, lev.R) and steps <= self.ops.FUSED_MAX_SWEEPS)

    def _turnaround(self, l, steps, omega):
        """Post-smoothing of one visit of level l and pre-smoothing of the next, with the restriction, in one pass."""
        lev, nxt = self.levels[l], self.levels[l + 1]
        self.ops.stencil_smooth_turnaround(lev.A, lev.x, lev.b, omega, steps, steps, lev.tmp,
                                           prolong=(lev.P, nxt.x), restrict=(lev.R, nxt.b))
        lev.x, lev.tmp = lev.tmp, lev.x

    def residual_norm(self, want_vector=True):
        """||b - A x||_2 on the fine level (Multigrid.py:62-63); one 8-byte D2H copy."""
        if self.cycle_values != "f64":
            raise ValueError("a hierarchy with cycle_values=%r is a preconditioner, not the operator of the outer iteration: "
                             "its sweeps read rounded values, so this would be the residual of A32 x = b.  Use it through "
                             "CG.solve / GMRES.solve(preconditioner=H), which take the residual with their own fp64 "
                             "operator" % (self.cycle_values,))
        lev = self.levels[0]
        self.ops.csr_residual_norm2(lev.A, lev.x, lev.b, self.outer_r if want_vector else None,
                               self.partials, self.norm2)
        return math.sqrt(self.norm2.item())

    def check_smoothers(self):
        """Raise if a wavefront Gauss-Seidel band of any level ever gave up waiting for its predecessor
        (gs_wave.hip then leaves a wrong iterate behind and sets a flag).  One 4-byte D2H read per level that
        has run the wavefront kernel: call it where the host synchronises anyway (after the residual norm of an
        outer iteration, after a graph replay)."""
        for lev in self.levels[:-1]:
            self._ask("stencil_gs_check", lev.A)

    def prepare_smoother(self, smoother, gs_mode="lexicographic", l_from=0, gs_sweep=("forward", "forward"), *,
                         cheby_lmax=None, cheby_ratio=None, line_dir=None, line_order=None, line_band=None):
        """Everything a Gauss-Seidel cycle would otherwise do lazily on its first sweep -- the wavefront kernel's eligibility
        test (a device -> host read) and work buffer, the level schedules -- from level l_from down, for every direction
        gs_sweep uses: nothing of it may happen while a hipGraph is being captured.
        Chebyshev: the bound lmax of D^-1 A per level -- cheby_lmax: None = its Gershgorin bound max_i sum_j |a_ij| / |a_ii|
        (never below the true lambda_max: no safety factor, the step cannot diverge), a float, or one value per smoothed
        level -- and lambda_min = lmax / cheby_ratio (default CHEBY_RATIO); the coefficient tables follow from them on the
        host.  rebuild_numeric() renews both.
        Line: the factored tridiagonal systems of every smoothed level for the directions of line_dir ("x" | "y" | "xy",
        default "xy") -- per level and direction two launches and one flag read --, and line_order ("zebra" | "jacobi",
        default "zebra").  A level that cannot run it raises a ValueError that names the level and the reason: no 3x3 grid
        geometry, rows that are no whole lines, a single line, an entry that couples two x-lines, a zero pivot.
        line_band (1 | 2 | 3; None: the band in use, 1 at first) is the largest half-bandwidth a level's line systems may
        have: per level and direction the smallest p <= line_band whose (2 p + 1)^2 window holds the level's offsets is used
        -- tridiagonal systems (p = 1) on 5-, 7- and 9-point levels, pentadiagonal (2) on the 25-point and heptadiagonal (3) on
        the 49-point Galerkin levels of learned or L2-type transfers.  Entries of a level outside the lines only enter
        through the residual; with wide stencils the lines of one zebra colour are still coupled, a colour is then a
        block-Jacobi step.  A level whose offsets fit no window up to line_band is refused with the window in the message.
        rebuild_numeric() renews the factors."""
        self._prepare(smoother, cheby_lmax, cheby_ratio, line_dir, line_order, line_band)
        if smoother != "GaussSeidel":
            return
        dirs = []
        for sw in gs_sweep_pair(gs_sweep):
            dirs += [d for d in _directions(sw) if d not in dirs]
        for l in range(l_from, len(self.levels) - 1):
            for d in dirs:
                if self._wavefront_gs(l, gs_mode, d):
                    self.ops.stencil_gs(self.levels[l].A, self.levels[l].tmp, self.levels[l].b, 0)
                else:
                    self.gs_schedule(l, gs_mode, d)

    def captured_cycle(self, smoother, steps, omega, gs_mode, gs_sweep=("forward", "forward"), shape="V", *,
                       cheby_lmax=None, cheby_ratio=None, line_dir=None, line_order=None, line_band=None, k_inner="gcr"):
        """The same launch sequence as cycle(), captured once into a hipGraph and replayed (one graph per sweep pair and
        cycle shape, and per k_inner of a K-cycle)."""
        pair = gs_sweep_pair(gs_sweep)
        cycle_children(shape)
        krylov = (k_inner_name(k_inner),) if shape in KRYLOV_SHAPES else ()
        self._prepare(smoother, cheby_lmax, cheby_ratio, line_dir, line_order, line_band)   # (before the key and the capture)
        if krylov:
            self._prepare_kcycle()
        key = (smoother, steps, omega, gs_mode, pair, shape) + krylov + self._smoother_key(smoother)
        g = self._graphs.get(key)
        if g is None:
            self.prepare_smoother(smoother, gs_mode, gs_sweep=pair)
            g = self._graphs[key] = capture_cycle(self.ops, self.levels, swap_from=1, run=lambda: self.cycle(
                smoother, steps, omega, gs_mode, gs_sweep=pair, shape=shape, k_inner=k_inner))
        return g

    def twin_bytes(self):
        """Bytes of the storage twins of every level's A, P and R at the width they have (fp32 value streams count 4 B a
        value): what the cycle's launches stream, next to the CSR arrays memory_bytes() counts -- those stay fp64 whatever
        cycle_values is, the Galerkin products and rebuild_numeric read them.  The census tables of the grid views (twins.py:
        census_table; 4 B an entry) are counted here and not in StencilTwin.bytes(), which bench.py reads as the traffic of
        one sweep: no sweep reads a table, a wave of a fused register pass reads four words of each."""
        tot = 0
        for lev in self.levels:
            for M in (lev.A, lev.P, lev.R):
                for name in ("patterns", "sell", "packed", "dia"):
                    T = getattr(M, name, None) if M is not None else None
                    tot += 0 if T is None else T.bytes()
                for name in ("stencil", "prolong", "restrict"):
                    census = getattr(getattr(M, name, None), "census", None)
                    tot += 0 if census is None else 4 * census.numel()
        return tot

    @staticmethod
    def _csr_model_bytes(M):
        """One pass over M in the byte model of cycle_bytes: 4 B column and 8 B value per entry -- 4 B where the twin the
        sweeps read stores fp32 values -- and the row pointers."""
        S = getattr(M, "sell", None)
        narrow = S is not None and getattr(S, "values", "f64") == "f32"
        return (8 if narrow else 12) * M.nnz + 4 * (M.shape[0] + 1)

    def memory_bytes(self):
        tot = 0
        for lev in self.levels:
            tot += lev.A.bytes() + (4 + (lev.d is not None) + (0 if lev.kc is None else len(lev.kc))) * 8 * lev.n
            tot += 0 if lev.line is None else sum(8 * (2 * lev.line_band[d] + 1) * lev.n for d in lev.line if d != "W")
            for M in (lev.P, lev.R, lev.RA):
                if M is not None:
                    tot += M.bytes()
        if self.kscal is not None:                     # (K-cycle: the scalars of the accelerated levels and the steps' scratch)
            tot += 8 * (sum(s.numel() for s in self.kscal[1:]) + self.kpartials.numel())
        return tot + self.coarse.bytes_per_apply()

    def cycle_bytes(self, steps):
        """Algorithmic HBM bytes of one V(steps,steps) cycle: per level
        (2*steps+1) sweeps + restriction + prolongation; coarsest dense apply separately.  An operator whose SELL or DIA
        twin stores fp32 values (cycle_values="f32") counts 4 B a value."""
        tot = 0
        for lev in self.levels[:-1]:
            n, nnz = lev.n, lev.A.nnz
            nc = lev.P.shape[1]
            D = getattr(lev.A, "dia", None)
            a_bytes = self._csr_model_bytes(lev.A) - (4 * nnz if D is not None and getattr(D, "values", "f64") == "f32" else 0)
            tot += (2 * steps + 1) * (a_bytes + 24 * n)
            tot += self._csr_model_bytes(lev.R) + 8 * n + 8 * nc
            tot += self._csr_model_bytes(lev.P) + 8 * nc + 16 * n
        coarse = (1 + self.coarse_refine) * self.coarse.bytes_per_apply()
        return tot, coarse
