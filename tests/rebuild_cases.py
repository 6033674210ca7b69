"""TEST-ONLY helpers of the rebuild-state tests (tests/test_rebuild_state_*.py): the value sets and scenarios a hierarchy is
rebuilt through, the smoother configurations, and assert_same_state -- the comparison of everything Hierarchy.rebuild_numeric
has to bring to the new values with a hierarchy built from them.  Imported by nothing in the package.

Every case lives on the 65^2 grid (4225 rows) with three levels, 4225 -> 1089 -> 289: the smallest size at which level 0 gets a
DIA twin (DiaTwin.MIN_ROWS = 4096) and the tiled passes (ops.TILED_MIN_ROWS = 4096) while level 1 gets neither.

    const          poisson_2d_structured(64): 3 distinct values, row patterns and the stencil twin
    var44, var45   variable_coeff_poisson_2d_structured(64, seed): the same pattern, 12 034 distinct values, packed CSR and DIA
    jit, jit45     jittered_poisson_2d(64, seed=42), and the same with coeff_sigma=0.5, coeff_seed=45: 7-point rows

const and var* go with the tensor-product transfers (geometric_hierarchy_2d(65, 3)), jit* with the learned-like pseudo-L2
transfers of the block tests (block_cg_ref.learned_like_hierarchy(65, 3)), whose Galerkin levels have 25- and 49-point rows."""
import functools

import numpy as np
import scipy.sparse as sp
import torch

import block_cg_ref as C
from learnmultigrid_amd import problems as P, smoothing
from oracle import kernels as K

M, LEVELS = 64, 3
SIZES = [4225, 1089, 289]
RTOL, FLOOR = 1e-10, 1e-14           # the project's standing bound for cycles (tests/test_amg_gpu.py)
NORM_RTOL = 1e-13                    # ... and for the squared norm of a residual between two storage formats

_MAKE = {"const": lambda m: P.poisson_2d_structured(m)[0],
         "var44": lambda m: P.variable_coeff_poisson_2d_structured(m, seed=44)[0],
         "var45": lambda m: P.variable_coeff_poisson_2d_structured(m, seed=45)[0],
         "jit": lambda m: P.jittered_poisson_2d(m, seed=42)[0],
         "jit45": lambda m: P.jittered_poisson_2d(m, seed=42, coeff_sigma=0.5, coeff_seed=45)[0]}

# name -> (the value sets the hierarchy goes through, whether the rebuilt hierarchy has the twin kinds of a fresh one)
SCENARIOS = {"var44-var45": (("var44", "var45"), True),
             "const-var45": (("const", "var45"), True),
             "var44-const": (("var44", "const"), False),
             "jit-jit45": (("jit", "jit45"), True),
             "const-var45-const-var45": (("const", "var45", "const", "var45"), True),
             "const-const": (("const", "const"), True)}
LINE_SCENARIOS = ("var44-var45", "const-var45")      # the Line smoother: one where the twin kinds stay, one where they change

# name -> (smoother, steps, omega, gs_mode, gs_sweep, shape, keywords of prepare_smoother / cycle / captured_cycle)
FWD = ("forward", "forward")
CONFIGS = {"jacobi-V": ("Jacobi", 2, 0.8, "lexicographic", FWD, "V", {}),
           "jacobi-W": ("Jacobi", 2, 0.8, "lexicographic", FWD, "W", {}),
           "jacobi-F": ("Jacobi", 2, 0.8, "lexicographic", FWD, "F", {}),
           "cheby-2": ("Chebyshev", 2, 1.0, "lexicographic", FWD, "V", {}),
           "cheby-3": ("Chebyshev", 3, 1.0, "lexicographic", FWD, "V", {}),
           "gs-lex-forward": ("GaussSeidel", 1, 1.0, "lexicographic", FWD, "V", {}),
           "gs-lex-symmetric": ("GaussSeidel", 1, 1.0, "lexicographic", ("symmetric", "symmetric"), "V", {}),
           "gs-multicolor": ("GaussSeidel", 1, 1.0, "multicolor", FWD, "V", {}),
           "gs-multicolor-device": ("GaussSeidel", 2, 1.0, "multicolor_device", ("forward", "backward"), "V", {})}
LINE_CONFIG = ("Line", 1, 1.0, "lexicographic", FWD, "V", {"line_dir": "x", "line_order": "zebra"})

TWINS = ("patterns", "stencil", "prolong", "restrict", "packed", "dia", "sell")


@functools.lru_cache(maxsize=None)
def matrix(name, m=M):
    """The operator of a value set: canonical CSR with int32 indices, read-only.  m: elements per side, for the tests
    without a device that need a level 0 below the size from which a level's geometry is read from its grid twin."""
    A = K.as_csr(sp.csr_matrix(_MAKE[name](m)))
    assert A.shape == ((m + 1) ** 2, (m + 1) ** 2) and A.has_canonical_format
    for a in (A.data, A.indices, A.indptr):
        a.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _family(learned, m):
    return tuple(C.learned_like_hierarchy(m + 1, LEVELS) if learned else P.geometric_hierarchy_2d(m + 1, LEVELS))


def transfers(name, m=M):
    """The transfers that go with a value set (one tuple per family, shared by its members)."""
    return _family(name.startswith("jit"), m)


def scenario(name):
    """(matrices, transfers, same_kinds) of a scenario.  Checked on the host: every value set of it has the index arrays of
    the first -- what rebuild_numeric requires -- and the transfers of the first."""
    chain, same_kinds = SCENARIOS[name]
    mats = [matrix(v) for v in chain]
    for v, A in zip(chain, mats):
        assert np.array_equal(A.indptr, mats[0].indptr) and np.array_equal(A.indices, mats[0].indices), (name, v)
        assert transfers(v) is transfers(chain[0]), (name, v)
    return mats, list(transfers(chain[0])), same_kinds


def values(A):
    """The values of a value set as a new CPU tensor (what rebuild_numeric takes, after a move to the device)."""
    return torch.from_numpy(A.data.copy())


@functools.lru_cache(maxsize=None)
def rhs(n=SIZES[0], seed=7):
    b = np.random.default_rng(seed).standard_normal(n)
    b.setflags(write=False)
    return b


def vector(n, seed, device):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(n)).to(device)


def twin_kinds(Mx):
    """Which storage twins a matrix holds, in the order of TWINS (none for a matrix on CPU tensors)."""
    return tuple(t for t in TWINS if getattr(Mx, t, None) is not None)


def twin_widths(Mx):
    """How the twins that can narrow store their values: {"sell" | "dia": "f64" | "f32"} of those a matrix holds."""
    return {t: getattr(Mx, t).values for t in ("sell", "dia") if getattr(Mx, t, None) is not None}


def level_kinds(H):
    """Per level the twin kinds of (A, P, R)."""
    return [tuple(() if Mx is None else twin_kinds(Mx) for Mx in (lev.A, lev.P, lev.R)) for lev in H.levels]


def within_cycle_bound(got, want, b_norm):
    """The largest |got - want| / (RTOL |want| + FLOOR ||b||): at most 1 within the project's bound for cycles."""
    return float(((got - want).abs() / (RTOL * want.abs() + FLOOR * b_norm)).max())


def _sync(H):
    if H.device.type == "cuda":
        torch.cuda.synchronize()


def _nan(n, device, count):
    return (torch.full((n,), float("nan"), dtype=torch.float64, device=device) for _ in range(count))


def _sweeps(o, A, x, b):
    """(A x, one Jacobi sweep, b - A x, its squared norm) through the ops module o, on whatever twin A has."""
    n, dev = A.shape[0], x.device
    y, xj, r = _nan(n, dev, 3)
    partials = torch.zeros(o.partials_count(n), dtype=torch.float64, device=dev)
    norm2 = torch.zeros(1, dtype=torch.float64, device=dev)
    o.csr_spmv(A, x, y)
    o.csr_jacobi(A, x, b, 0.8, xj)
    o.csr_residual_norm2(A, x, b, r, partials, norm2)
    return y, xj, r, float(norm2.item())


def _fused_pass(o, A, x, b):
    """(one Jacobi sweep, the residual after it) as one fused pass where A runs them (the stencil views and the DIA twin
    are read by nothing else), else None."""
    if not smoothing.ask(o, "stencil_smooth_available", A):
        return None
    out, r = _nan(A.shape[0], x.device, 2)
    o.stencil_smooth(A, x, b, 0.8, 1, out, r)
    return out, r


def assert_same_state(H, F, same_kinds=True):
    """The rebuilt hierarchy H against F = Hierarchy(to_values, the same transfers, the same keywords), after the same
    prepare_smoother calls on both.  Per level: the CSR arrays of A and the values of R A bit for bit; the inverse diagonal
    wherever either holds one; which storage twins A, P and R have (equal when same_kinds, returned either way); one SpMV,
    one Jacobi sweep and one residual on A against the same calls on A.plain() (fp32 twins: on the rounded view they stand
    for, A.cycle_source()), and the fused pass where A has one -- every twin is lossless, so a twin that
    still holds old values shows here even on a level the smoother under test never sweeps.  Then the coarse solver (kind,
    the measured coarse_refine and coarse_residual, one application bit for bit) and what the stateful smoothers keep: the
    Chebyshev bounds, ratio and coefficient tables, the line geometry and factors.  Returns (kinds of H, kinds of F)."""
    o = H.ops
    _sync(H)
    assert H.sizes == F.sizes and H.cycle_values == F.cycle_values
    kinds_h, kinds_f = level_kinds(H), level_kinds(F)
    for l, (h, f) in enumerate(zip(H.levels, F.levels)):
        for name in ("rowptr", "colidx", "vals"):
            assert torch.equal(getattr(h.A, name), getattr(f.A, name)), "level %d: A.%s" % (l, name)
        assert (h.RA is None) == (f.RA is None), l
        if h.RA is not None:
            assert torch.equal(h.RA.vals, f.RA.vals), "level %d: RA.vals" % l
        if h.dinv is not None or f.dinv is not None:
            fresh = o.csr_inverse_diagonal(F._cycle_source(f.A))
            for who, lev in (("rebuilt", h), ("fresh", f)):
                assert lev.dinv is None or torch.equal(lev.dinv, fresh), "level %d: dinv of the %s hierarchy" % (l, who)
        assert kinds_h[l][1:] == kinds_f[l][1:], "level %d: twins of P, R %s, fresh %s" % (l, kinds_h[l][1:], kinds_f[l][1:])
        if same_kinds:
            assert kinds_h[l][0] == kinds_f[l][0], "level %d: twins of A %s, fresh %s" % (l, kinds_h[l][0], kinds_f[l][0])
        x, b = vector(h.n, 100 + l, H.device), vector(h.n, 200 + l, H.device)
        # what the twins stand for, without twins: the CSR arrays, or -- fp32 twins -- the rounded view of them
        assert h.A.twin_values == f.A.twin_values, "level %d: twins hold %s, fresh %s" % (l, h.A.twin_values, f.A.twin_values)
        wh, wf = twin_widths(h.A), twin_widths(f.A)
        assert all(wh[t] == wf[t] for t in set(wh) & set(wf)), (l, wh, wf)
        plain = h.A.cycle_source() if h.A.twin_values == "f32" else h.A.plain()
        want = _sweeps(o, plain, x, b)
        after, = _nan(h.n, H.device, 1)
        o.csr_residual_norm2(plain, want[1], b, after, None, None)             # the residual after the Jacobi sweep
        for who, A in (("rebuilt", h.A), ("fresh", f.A)):
            where = "level %d, %s twins %s: " % (l, who, twin_kinds(A))
            got = _sweeps(o, A, x, b)
            for what, g, w in zip(("spmv", "jacobi", "residual"), got, want):
                assert torch.equal(g, w), where + what + " differs from the plain CSR sweep"
            assert abs(got[3] - want[3]) <= NORM_RTOL * want[3], (where, got[3], want[3])
            fused = _fused_pass(o, A, x, b)
            if fused is not None:
                assert torch.equal(fused[0], want[1]) and torch.equal(fused[1], after), where + "the fused pass differs"
        # the Gauss-Seidel schedules both hold (the one of kind multicolor_device sweeps a copy of the values)
        for key in sorted(set(h.gs_sched) & set(f.gs_sched), key=repr):
            xh, xf = x.clone(), x.clone()
            o.csr_gs_schedule(h.A, xh, b, h.gs_sched[key], 1)
            o.csr_gs_schedule(f.A, xf, b, f.gs_sched[key], 1)
            assert torch.equal(xh, xf) and not torch.equal(xh, x), "level %d: sweep on the schedule %r" % (l, key)
    # the coarse solver
    assert H.coarse.kind == F.coarse.kind
    assert H.coarse_refine == F.coarse_refine
    assert getattr(H, "coarse_residual", None) == getattr(F, "coarse_residual", None)
    nc = H.levels[-1].n
    bc = vector(nc, 300, H.device)
    xh, xf = (torch.full((nc,), float("nan"), dtype=torch.float64, device=H.device) for _ in range(2))
    H.coarse.apply(bc, xh)
    F.coarse.apply(bc, xf)
    assert torch.equal(xh, xf) and bool(torch.isfinite(xh).all()), "coarse.apply"
    # Chebyshev: bounds, ratio, tables
    assert H.cheby_key() == F.cheby_key()
    if F._cheby is not None:
        assert H._cheby["args"] == F._cheby["args"] and H._cheby["lmax"] == F._cheby["lmax"]
        for l, degree in sorted(set(H._cheby["coef"]) | set(F._cheby["coef"])):
            assert H._cheby_coef(l, degree) == F._cheby_coef(l, degree), (l, degree)
    # Line: geometry and factors
    assert H.line_key() == F.line_key() and H._line_band == F._line_band
    for l, (h, f) in enumerate(zip(H.levels[:-1], F.levels[:-1])):
        assert (h.line is None) == (f.line is None), l
        if f.line is None:
            continue
        assert h.line_band == f.line_band and sorted(h.line) == sorted(f.line) and h.line["W"] == f.line["W"], l
        for d in (d for d in f.line if d != "W"):
            hf, ff = ((fac,) if torch.is_tensor(fac) else tuple(fac) for fac in (h.line[d], f.line[d]))
            assert len(hf) == len(ff) and all(torch.equal(a, b) for a, b in zip(hf, ff)), "level %d: %s-line factors" % (l, d)
    _sync(H)
    return kinds_h, kinds_f
