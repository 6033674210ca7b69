"""TEST-ONLY helpers of the tests on operators that are NOT numbered line by line on a grid (tests/test_reordered_*.py):
the numberings (Morton, random, "mixed": fine level in grid order, coarse levels random), the symmetric renumbering of a
problem and of its transfers, the four problem kinds, and the tolerance rule of every history and iterate comparison there.

The tolerance rule.  A residual norm h is compared with the reference's w as |h - w| <= RTOL * w + atol with
atol = (k + 2) * eps * || |A| |x_ref| + |b| ||_2, k the longest row of A and x_ref the reference's iterate at that entry: the
textbook rounding bound of ONE evaluated residual b - A x (k products, k additions to b, Higham, Accuracy and Stability,
section 3.5: |fl(b - A x) - (b - A x)| <= gamma_(k+1) (|A||x| + |b|) componentwise, taken in the 2-norm).  It is derived, not
tuned: two correct implementations that differ in summation order cannot be asked for less, and on a renumbered 33^2
variable-coefficient problem the ops shim and oracle.vcycle_ref.HoistedVCycle already differ by 1.85e-10 relative after five
Gauss-Seidel cycles, where the norm is at its rounding floor.  Iterates are compared as |x - x_ref| <= RTOL * max|x_ref|."""
import functools

import numpy as np
import scipy.sparse as sp

from block_cg_ref import learned_like_hierarchy
from learnmultigrid_amd import problems as P
from line_band_ref import symmetrised
from oracle import kernels as K

RTOL = 1e-10
EPS = float(np.finfo(np.float64).eps)
KINDS = ("const", "var", "learned", "sym")
NUMBERINGS = ("morton", "random", "mixed")
RANDOM_SEED = 5                       # level l is drawn with seed RANDOM_SEED + l
CYCLES, STEPS, OMEGA = 6, 2, 0.8      # of every history: 6 cycles of 2 sweeps, weighted Jacobi at 0.8
SMOOTHERS = ("Jacobi", "GaussSeidel")
# (kind, numbering, m, levels) of every hierarchy whose history the device tests compare with the oracle; the CPU tests hold
# the reference pair (ops shim, HoistedVCycle) to a tenth of the rule's atol on each of them
CYCLE_CASES = tuple((k, nb, 64, 3) for k in ("const", "var", "learned") for nb in NUMBERINGS) + (("var", "random", 256, 4),)
OTHER_CASES = (("var", "morton", 128, 2),        # the coarse solvers: a coarsest level of 4225 rows
               ("var", "morton", 32, 3), ("var", "random", 32, 3),                  # the solver front end
               ("sym", "random", 64, 3),         # the Krylov front ends
               ("learned", "random", 64, 3))     # solve_many


def morton_order(side):
    """The nodes y * side + x of a side x side grid sorted by the interleaved bits of (x, y) (x the lowest bit)."""
    side = int(side)
    idx = np.arange(side * side, dtype=np.int64)
    x, y = idx % side, idx // side
    code = np.zeros(side * side, dtype=np.int64)
    for bit in range(max(side - 1, 1).bit_length()):
        code |= ((x >> bit) & 1) << (2 * bit)
        code |= ((y >> bit) & 1) << (2 * bit + 1)
    return np.argsort(code, kind="stable")


def random_order(n, seed):
    return np.random.default_rng(seed).permutation(int(n))


def orders_for(numbering, side, levels, seeds=None):
    """One order per level of the `levels` grids below a side^2 fine grid (None: grid order).  seeds: the seed of every
    level's random draw, RANDOM_SEED + l by default."""
    sizes = P.level_sizes(side, levels)
    seeds = [RANDOM_SEED + l for l in range(levels)] if seeds is None else list(seeds)
    if numbering == "grid":
        return [None] * levels
    if numbering == "morton":
        return [morton_order(s) for s in sizes]
    if numbering == "random":
        return [random_order(s * s, seeds[l]) for l, s in enumerate(sizes)]
    if numbering == "mixed":
        return [None] + [random_order(s * s, seeds[l]) for l, s in enumerate(sizes) if l >= 1]
    raise ValueError("numbering must be 'grid' or one of %s, got %r" % (NUMBERINGS, numbering))


def _take(M, rows, cols):
    M = sp.csr_matrix(M)
    if rows is not None:
        M = M[rows]
    if cols is not None:
        M = M[:, cols]
    return K.as_csr(sp.csr_matrix(M))


def reorder(A, hierarchy, rhs, orders):
    """orders[l]: the new numbering of level l -- new unknown i is old unknown orders[l][i] -- or None to keep it.
    Returns (A[o0][:, o0], [P_l[o_l][:, o_(l+1)]], rhs[o0]) as canonical CSR (sorted rows, int32 indices, fp64 values)."""
    if len(orders) != len(hierarchy) + 1:
        raise ValueError("%d levels need %d orders, got %d" % (len(hierarchy) + 1, len(hierarchy) + 1, len(orders)))
    Ap = _take(A, orders[0], orders[0])
    Hp = [_take(Pl, orders[l], orders[l + 1]) for l, Pl in enumerate(hierarchy)]
    b = np.asarray(rhs, dtype=float).reshape(-1)
    return Ap, Hp, (b.copy() if orders[0] is None else b[orders[0]])


def unpermute(x, order):
    """The vector of a reordered run in the old numbering."""
    x = np.asarray(x).reshape(-1)
    if order is None:
        return x.copy()
    out = np.empty_like(x)
    out[order] = x
    return out


@functools.lru_cache(maxsize=None)
def problem(kind, m, levels):
    """(A, hierarchy, rhs) in grid order on the (m + 1)^2 grid with `levels` grids, made once and shared (do not write to them):
      "const"    poisson_2d_structured with geometric_hierarchy_2d
      "var"      variable_coeff_poisson_2d_structured(seed=44) with geometric_hierarchy_2d
      "learned"  "var" with learned_like(kron(pseudo_l2, pseudo_l2), 43 + l) transfers: 25- and 49-entry Galerkin rows
      "sym"      the symmetric interior block of the MG-PCG tests (block_cg_ref.problem at any size: jittered_poisson_2d(seed=42)
                 with the boundary rows and columns eliminated, line_band_ref.symmetrised) and its learned-like transfers"""
    side = m + 1
    if kind == "const":
        A, rhs = P.poisson_2d_structured(m)
        hier = P.geometric_hierarchy_2d(side, levels)
    elif kind == "var":
        A, rhs = P.variable_coeff_poisson_2d_structured(m, seed=44)
        hier = P.geometric_hierarchy_2d(side, levels)
    elif kind == "learned":
        A, rhs = P.variable_coeff_poisson_2d_structured(m, seed=44)
        hier = learned_like_hierarchy(side, levels, 43)
    elif kind == "sym":
        A, rhs = P.jittered_poisson_2d(m, seed=42)
        A = symmetrised(A)
        hier = learned_like_hierarchy(side, levels, 43)
    else:
        raise ValueError("kind must be one of %s, got %r" % (KINDS, kind))
    A = K.as_csr(A)
    hier = tuple(K.as_csr(sp.csr_matrix(p)) for p in hier)
    rhs = np.ascontiguousarray(rhs, dtype=float).reshape(-1)
    rhs.setflags(write=False)
    return A, hier, rhs


@functools.lru_cache(maxsize=None)
def reordered(kind, numbering, m, levels, seeds=None):
    """problem(kind, m, levels) under `numbering`: (Ap, Hp, bp, orders), read-only, made once."""
    A, hier, rhs = problem(kind, m, levels)
    orders = orders_for(numbering, m + 1, levels, seeds)
    Ap, Hp, bp = reorder(A, list(hier), rhs, orders)
    bp.setflags(write=False)
    return Ap, Hp, bp, orders


# ---- the tolerance rule ------------------------------------------------------------------------------------------------------
def tolerances(A, x_ref, b):
    """atol of a residual norm taken at the reference's iterate x_ref: (k + 2) eps || |A||x_ref| + |b| ||_2."""
    A = sp.csr_matrix(A)
    k = int(np.diff(A.indptr).max())
    x = np.abs(np.asarray(x_ref, dtype=float).reshape(-1))
    return (k + 2) * EPS * float(np.linalg.norm(abs(A) @ x + np.abs(np.asarray(b, dtype=float).reshape(-1))))


def deviation(got, want, atols):
    """max_i |got_i - want_i| / atol_i: how much of the rounding bound a history uses (the rule adds RTOL * want to it)."""
    got, want, atols = (np.asarray(v, dtype=float).reshape(-1) for v in (got, want, atols))
    assert got.shape == want.shape == atols.shape, (got.shape, want.shape, atols.shape)
    return float(np.max(np.abs(got - want) / atols))


def assert_history(got, want, atols, what=""):
    """The rule on every entry.  Returns deviation(got, want, atols)."""
    got, want, atols = (np.asarray(v, dtype=float).reshape(-1) for v in (got, want, atols))
    assert got.shape == want.shape == atols.shape, (what, got.shape, want.shape, atols.shape)
    bad = np.abs(got - want) > RTOL * np.abs(want) + atols
    assert not bad.any(), "%s: entries %s: got %s, want %s, atol %s" % (what, np.flatnonzero(bad), got[bad], want[bad], atols[bad])
    return deviation(got, want, atols)


def assert_iterate(x, x_ref, what=""):
    """|x - x_ref| <= RTOL * max|x_ref|.  Returns max|x - x_ref| / max|x_ref|."""
    x, x_ref = np.asarray(x, dtype=float).reshape(-1), np.asarray(x_ref, dtype=float).reshape(-1)
    assert x.shape == x_ref.shape, (what, x.shape, x_ref.shape)
    err = float(np.max(np.abs(x - x_ref))) / float(np.max(np.abs(x_ref)))
    assert err <= RTOL, "%s: max|x - x_ref| = %.3e max|x_ref|" % (what, err)
    return err


def oracle_history(ref, A, b, cycles, **kw):
    """`cycles` cycles of `ref` (HoistedVCycle, ChebyCycle) from a zero guess: (norms, atols, iterates) with cycles + 1
    entries each -- ||b - A x|| of the oracle's residual, the rule's atol and the iterate, before the first and after every cycle."""
    A = K.as_csr(A)
    b = np.asarray(b, dtype=float).reshape(-1)
    x = np.zeros(A.shape[0])
    norms, atols, xs = [], [], []
    for c in range(cycles + 1):
        norms.append(float(np.sqrt(K.residual(A, x, b)[1])))
        atols.append(tolerances(A, x, b))
        xs.append(x.copy())
        if c < cycles:
            x = ref.cycle(x, b, **kw)
    return np.array(norms), np.array(atols), xs


@functools.lru_cache(maxsize=None)
def hoisted(kind, numbering, m, levels):
    """oracle.vcycle_ref.HoistedVCycle of reordered(kind, numbering, m, levels), made once."""
    from oracle.vcycle_ref import HoistedVCycle
    Ap, Hp, _, _ = reordered(kind, numbering, m, levels)
    return HoistedVCycle(Ap, Hp)


@functools.lru_cache(maxsize=None)
def reference(kind, numbering, m, levels, smoother):
    """oracle_history of CYCLES cycles of STEPS sweeps (Jacobi: OMEGA) on that hierarchy: computed once, shared, read only."""
    Ap, _, bp, _ = reordered(kind, numbering, m, levels)
    norms, atols, xs = oracle_history(hoisted(kind, numbering, m, levels), Ap, bp, CYCLES, smoother=smoother, steps=STEPS,
                                      omega=OMEGA)
    for v in [norms, atols] + xs:
        v.setflags(write=False)
    return norms, atols, xs


def hierarchy_history(H, b, cycles, smoother, steps, omega=1.0, graph=None, to=None, **kw):
    """The same from a Hierarchy (on CPU tensors with the ops shim, or on the device): (norms, final iterate).  graph: a
    captured cycle to replay in place of H.cycle.  to: moves a NumPy vector to the hierarchy's device (None: CPU tensors)."""
    import contextlib
    import torch
    fine = H.levels[0]
    bt = torch.from_numpy(np.ascontiguousarray(b, dtype=float).reshape(-1).copy())
    norms = []
    with (torch.cuda.stream(H.stream) if H.stream is not None else contextlib.nullcontext()):
        fine.b.copy_(bt if to is None else to(bt))
        fine.x.zero_()
        for c in range(cycles + 1):
            norms.append(H.residual_norm())
            if c < cycles:
                if graph is not None:
                    graph.launch()
                else:
                    H.cycle(smoother, steps, omega, **kw)
        x = H.levels[0].x.cpu().numpy().copy()
    return np.array(norms), x
