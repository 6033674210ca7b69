"""What a smoothing step launches: the names and keyword checks of the smoothers, and the launch sequences that the
hierarchy, the distributed cycle and the operator handles of torch.ops.lmg share -- like krylov.py written against an ops
module `o` handed in (the HIP kernels; a CPU shim in the host-logic tests).  The vectors come as any object `v` with the
attributes of a hierarchy level that the sequence uses (x, tmp, b, r, d, dinv); v.x and v.tmp swap after every pass.
One call per smoothing step: nothing here wraps a single launch."""
import math

import numpy as np
import scipy.sparse as sp


GS_SWEEPS = ("forward", "backward", "symmetric")       # pyamg's gauss_seidel(sweep=...)
# the orderings of a Gauss-Seidel sweep (gs_mode): the exact sweep, colour classes found on the host, and colour classes
# found on the device with the sweep on a sliced-ELL copy in colour order (ops.build_gs_schedule_device)
GS_MODES = ("lexicographic", "multicolor", "multicolor_device")


def gs_sweep_pair(gs_sweep):
    """(pre, post) smoothing directions of a Gauss-Seidel cycle from a pyamg sweep name (used for both) or a pair."""
    pair = (gs_sweep, gs_sweep) if isinstance(gs_sweep, str) else tuple(gs_sweep)
    if len(pair) != 2 or any(d not in GS_SWEEPS for d in pair):
        raise ValueError("gs_sweep must be one of %s or a (pre, post) pair of them, got %r" % (GS_SWEEPS, gs_sweep))
    return pair


def gs_mode_name(gs_mode, what="gs_mode"):
    """gs_mode as it is, or a ValueError (reads no state: the Krylov solvers check their keyword with it before any setup)."""
    if gs_mode not in GS_MODES:
        raise ValueError("%s must be one of %s, got %r" % (what, GS_MODES, gs_mode))
    return gs_mode


def _directions(sweep):
    return ("forward", "backward") if sweep == "symmetric" else (sweep,)


def chebyshev_coefficients(lmax, ratio, degree):
    """The (a_k, c_k), k = 0 .. degree - 1, of one Chebyshev smoothing step on [lmax / ratio, lmax] for D^-1 A:
        d_k = a_k d_(k-1) + c_k D^-1 (b - A x_k),   x_(k+1) = x_k + d_k,
    the three-term recurrence of the shifted and scaled Chebyshev polynomial (error polynomial of one step:
    T_S((theta - lambda) / delta) / T_S(sigma)), in Python floats."""
    lmax, ratio, degree = float(lmax), float(ratio), int(degree)
    if not (ratio > 1.0 and math.isfinite(ratio)):
        raise ValueError("cheby_ratio must be a finite number > 1 (lambda_min = lambda_max / cheby_ratio), got %r" % (ratio,))
    if not (lmax > 0.0 and math.isfinite(lmax)):
        raise ValueError("the Chebyshev smoother needs a finite bound lambda_max > 0 for D^-1 A, got %r" % (lmax,))
    if degree < 1:
        raise ValueError("the Chebyshev smoother needs a degree (smooth_steps) >= 1, got %r" % (degree,))
    lmin = lmax / ratio
    theta = (lmax + lmin) / 2
    delta = (lmax - lmin) / 2
    sigma = theta / delta
    rho = 1 / sigma
    coef = [(0.0, 1 / theta)]
    for _ in range(1, degree):
        rho_k = 1 / (2 * sigma - rho)
        coef.append((rho_k * rho, 2 * rho_k / delta))
        rho = rho_k
    return coef


CHEBY_RATIO = 4.0       # lambda_max / lambda_min: the oscillatory modes of D^-1 A under full coarsening in two dimensions
LINE_DIRS = ("x", "y", "xy")          # the line_dir of the "Line" smoother: the systems one step solves, in this order
LINE_ORDERS = ("zebra", "jacobi")     # its line_order: even systems then odd ones with a fresh residual, or all from one
STATEFUL = ("Chebyshev", "Line")      # the smoothers with keywords: Hierarchy.prepare_smoother keeps state for them


def line_config(line_dir=None, line_order=None):
    """(line_dir, line_order) with the defaults ("xy", "zebra") filled in, or a ValueError (reads no state: the solver
    classes check their keywords with it before any setup)."""
    line_dir = "xy" if line_dir is None else line_dir
    line_order = "zebra" if line_order is None else line_order
    if line_dir not in LINE_DIRS:
        raise ValueError("line_dir must be one of %s, got %r" % (LINE_DIRS, line_dir))
    if line_order not in LINE_ORDERS:
        raise ValueError("line_order must be one of %s, got %r" % (LINE_ORDERS, line_order))
    return line_dir, line_order


LINE_BANDS = (1, 2, 3)                # its line_band: the largest half-bandwidth of a level's line systems (3x3, 5x5, 7x7 stencils)


def line_band_value(line_band=None):
    """line_band as an int, None as it is (the caller's default), or a ValueError (reads no state, like line_config)."""
    if line_band is None:
        return None
    if isinstance(line_band, bool) or line_band not in LINE_BANDS:
        raise ValueError("line_band must be one of %s, got %r" % (LINE_BANDS, line_band))
    return int(line_band)


def chebyshev_degree(steps):
    """The degree of a Chebyshev smoothing step (the smooth_steps of the solvers, the `steps` of a cycle), or a ValueError."""
    if steps < 1:
        raise ValueError("the Chebyshev smoother needs smooth_steps >= 1 (the degree), got %r" % (steps,))


def smoother_options(smoother, steps, *, cheby_lmax=None, cheby_ratio=None, line_dir=None, line_order=None, line_band=None):
    """The keywords of `smoother` as the solver classes hand them to Hierarchy.prepare_smoother(smoother, **options), or a
    ValueError for a value it cannot take; the keywords of another smoother are not looked at ({} for Jacobi and Gauss-Seidel).
    Reads no state and touches no device: every solver class calls it before any setup.  What a keyword left None means to
    a solver class is decided here: "Line" runs ("xy", "zebra") with line_band 1 (to the hierarchy itself None is "what is
    prepared"), "Chebyshev" keeps the bounds the hierarchy has (its defaults at first)."""
    if smoother == "Chebyshev":
        chebyshev_degree(steps)
        if cheby_ratio is not None and not float(cheby_ratio) > 1.0:
            raise ValueError("cheby_ratio must be > 1 (lambda_min = lambda_max / cheby_ratio), got %r" % (cheby_ratio,))
        return {"cheby_lmax": cheby_lmax, "cheby_ratio": cheby_ratio}
    if smoother == "Line":
        line_dir, line_order = line_config(line_dir, line_order)
        return {"line_dir": line_dir, "line_order": line_order, "line_band": 1 if line_band is None else line_band_value(line_band)}
    return {}


def line_ops(o, p):
    """(factor(A, W, dir), solve(W, dir, first, step, fac, r, omega, x)) of line systems with half-bandwidth p: the
    tridiagonal kernels for p = 1, the banded ones otherwise (they round differently and stay two sets of kernels)."""
    if p == 1:
        return o.line_factor, o.line_solve
    return (lambda A, W, d: o.line_factor_banded(A, W, d, p)), (lambda W, d, *rest: o.line_solve_banded(W, d, p, *rest))


def line_half_steps(line_dir, line_order, reverse=False):
    """The launches of one "Line" smoothing step as (direction, first, step) of ops.line_solve, each after a fresh residual:
    per direction of line_dir the even systems then the odd ones (zebra) or all systems (jacobi).  reverse: the
    post-smoothing half -- directions and colours in the opposite order, which makes the cycle's smoothing halves adjoint
    to each other whenever A is symmetric."""
    colours = ((0, 2), (1, 2)) if line_order == "zebra" else ((0, 1),)
    out = [(d, first, step) for d in line_dir for (first, step) in colours]
    return out[::-1] if reverse else out


def ask(o, name, *args):
    """o.<name>(*args), or False where the ops module has no such name (an ops module leaves out what it does not offer)."""
    fn = getattr(o, name, None)
    return fn(*args) if fn is not None else False


def fused_passes(o, A, v, steps, omega, x_is_zero=False, want_residual=False, correction=None, restrict_to=None, coef=None):
    """`steps` Jacobi sweeps on A as fused passes of at most o.FUSED_MAX_SWEEPS sweeps each; the last pass writes v.r =
    b - A x (want_residual) or forms b_coarse = R (b - A x) without writing it (restrict_to = (R, b_coarse)); the first
    starts from x + P e (correction = (P, e)).  coef: a Chebyshev table -- its one step of degree `steps` as the one pass."""
    cheby = coef is not None
    run = o.stencil_cheby if cheby else o.stencil_smooth
    left = steps
    while left > 0:
        k = left if cheby else min(left, o.FUSED_MAX_SWEEPS)
        left -= k
        how = (coef,) if cheby else (omega, k)
        x_in = None if x_is_zero else v.x
        if correction is not None:
            run(A, v.x, v.b, *how, v.tmp, None, prolong=correction)
            correction = None
        elif restrict_to is not None and left == 0:
            run(A, x_in, v.b, *how, v.tmp, None, restrict=restrict_to)
        else:
            run(A, x_in, v.b, *how, v.tmp, v.r if (want_residual and left == 0) else None)
        v.x, v.tmp = v.tmp, v.x
        x_is_zero = False


def chebyshev_step(o, A, v, coef, x_is_zero=False):
    """One Chebyshev step with the table `coef` in place on v.x, per sweep v.r = b - A x, then d = a d + c D^-1 r and x += d."""
    for k, (a, c) in enumerate(coef):
        if k == 0 and x_is_zero:
            o.zero(v.x)
            o.cheby_update(a, c, v.dinv, v.b, v.d, v.x, first=True)     # b - A 0 = b
        else:
            o.csr_residual_norm2(A, v.x, v.b, v.r, None, None)
            o.cheby_update(a, c, v.dinv, v.r, v.d, v.x, first=(k == 0))


def wavefront_gs(o, A, direction="forward"):
    """Whether the exact sweep on A runs as the pipelined wavefront kernel (grid-stencil operators) in this direction."""
    return ask(o, "stencil_gs_available", A) if direction == "forward" else ask(o, "stencil_gs_available", A, direction)


def gauss_seidel(o, A, v, wavefront, schedule, steps, direction="forward"):
    """`steps` exact Gauss-Seidel sweeps in one direction, in place on v.x: the wavefront kernel where the caller found it to
    run (`wavefront`: wavefront_gs and whatever else it requires), otherwise the schedule of schedule(), only called then."""
    if direction not in ("forward", "backward"):
        raise ValueError("unknown Gauss-Seidel sweep direction %r" % (direction,))
    if wavefront:
        if direction == "forward":
            o.stencil_gs(A, v.x, v.b, steps)
        else:
            o.stencil_gs(A, v.x, v.b, steps, direction)
    else:
        o.csr_gs_schedule(A, v.x, v.b, schedule(), steps)


def gs_schedule(o, A, rowptr, colidx, kind, device, row_offset=0):
    """The Gauss-Seidel schedule (`kind`: "lexicographic" | "multicolor") of the square pattern in the host arrays (rowptr,
    colidx) for sweeps on A, prepared (o.gs_prepare: what the first sweep would otherwise allocate and read back -- never
    while a hipGraph is being captured).  row_offset: where the pattern's row 0 lies among the rows of A."""
    n = len(rowptr) - 1
    pat = sp.csr_matrix((np.ones(len(colidx), dtype=np.int8), colidx, rowptr), shape=(n, n))
    sched = o.build_gs_schedule(pat, kind, device)
    if row_offset:
        sched.d_rows += row_offset
    ask(o, "gs_prepare", A, sched)
    return sched
