"""Backward and symmetric Gauss-Seidel (-m gpu): the mirrored wavefront kernels of gs_wave.hip
(lmg_stencil_gs_sweep_backward), reversed level / colour schedules for every other matrix, and the
sweep keywords of the hierarchy and the solvers -- against pyamg's backward sweep restated by the
CPU oracle (orc_csr_gs_rows over rows n-1 .. 0), bitwise.
"""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from learnmultigrid_amd import ops, problems as P                # noqa: E402
from learnmultigrid_amd._lib import LmgError                     # noqa: E402
from oracle import kernels as K                                  # noqa: E402  (checker only)
from oracle import vcycle_ref as V                               # noqa: E402  (checker only)
from support import DEV, dev, galerkin9                          # noqa: E402


def backward_rows(n):
    return np.arange(n - 1, -1, -1, dtype=np.int32)


def oracle_backward(A, x, b, sweeps):
    rows = backward_rows(A.shape[0])
    for _ in range(sweeps):
        K.gs_rows(A, x, b, rows)
    return x


def grid_operator(nx, ny, kind="5pt", sym=False, var=False):
    """Operator of an ny-line x nx-column grid with identity (Dirichlet) rows on the boundary, columns untouched
    (sym=True: the symmetric interior block, couplings to boundary rows dropped).  var=True scales every interior row
    by one of six factors (6 interior patterns) and adds a row without its diagonal and an empty row."""
    n = nx * ny
    idx = np.arange(n)
    yy, xx = idx // nx, idx % nx
    inter = (xx > 0) & (xx < nx - 1) & (yy > 0) & (yy < ny - 1)
    if kind == "5pt":
        sten = ((-nx, -1.0), (-1, -1.0), (0, 4.0), (1, -1.0), (nx, -1.0))
    elif kind == "7pt":
        sten = ((-nx - 1, -0.5), (-nx, -1.0), (-1, -1.0), (0, 6.25), (1, -1.0), (nx, -1.0), (nx + 1, -0.5))
    else:
        sten = tuple((c * nx + d, 8.0 if c == d == 0 else -1.0 - 0.125 * (c + 2 * d)) for c in (-1, 0, 1) for d in (-1, 0, 1))
    scale = 1.0 + 0.25 * ((xx % 3) + 3 * (yy % 2)) if var else np.ones(n)
    rows, cols, vals = [idx[~inter]], [idx[~inter]], [np.ones((~inter).sum())]
    ri = idx[inter]
    for off, v in sten:
        c = ri + off
        keep = inter[c] if sym and off != 0 else np.ones(c.size, dtype=bool)
        rows.append(ri[keep])
        cols.append(c[keep])
        vals.append(v * scale[ri[keep]])
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    if var:
        A = A.tolil()
        A[nx + 5, :] = 0.0                                   # empty row
        A[3 * nx + 7, 3 * nx + 7] = 0.0                      # row without a diagonal entry
        A = sp.csr_matrix(A)
        A.eliminate_zeros()
    return K.as_csr(A)


CASES = {
    "5pt_40x40": lambda: K.as_csr(P.poisson_2d_structured(39)[0]),             # W < 64: register bands only
    "5pt_sym_130x70": lambda: grid_operator(130, 70, sym=True),                # non-square, symmetric interior block
    "5pt_3x50": lambda: grid_operator(3, 50),                                  # smallest line stride
    "5pt_64x97": lambda: grid_operator(64, 97),                                # smallest LDS line stride, 97 lines
    "5pt_var_203x77": lambda: grid_operator(203, 77, var=True),               # several pattern ids, empty / diagless rows
    "7pt_150x150": lambda: grid_operator(150, 150, "7pt"),
    "7pt_sym_81x45": lambda: grid_operator(81, 45, "7pt", sym=True),
    "9pt_galerkin_151": lambda: galerkin9(151),                                # 32-line LDS bands, division path
    "9pt_galerkin_33": lambda: galerkin9(33),
    "9pt_100x45": lambda: grid_operator(100, 45, "9pt"),
    "9pt_var_70x65": lambda: grid_operator(70, 65, "9pt", var=True),
}
WANT_MASK = {"5pt": 0x0BA, "7pt": 0x1BB, "9pt": 0x1FF}


@pytest.mark.parametrize("name", sorted(CASES))
def test_backward_wavefront_bit_exact_under_every_forcing(name):
    """1 - 7 backward sweeps (crossing the 4 sweeps of one launch) in each forced configuration -- register / LDS bands,
    one sweep or up to four per launch -- bitwise against the oracle's rows n-1 .. 0, and all configurations alike."""
    A = CASES[name]()
    n = A.shape[0]
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack()
    S = dA.stencil
    assert S is not None and S.umask == WANT_MASK[name[:3]], (name, None if S is None else hex(S.umask))
    assert n % S.W == 0 and ops.stencil_gs_available(dA) and ops.stencil_gs_available(dA, "backward"), name
    if name == "5pt_var_203x77":
        assert S.npat > 6
    rng = np.random.default_rng(17)
    x0, b = rng.standard_normal(n), rng.standard_normal(n)
    db = dev(b)
    want = {0: x0.copy()}
    for s in range(1, 8):
        want[s] = oracle_backward(A, want[s - 1].copy(), b, 1)
    try:
        for lds in (-1, 0, 1):
            for ms in (1, 4):
                ops.tune_set("gsw_lds", lds)
                ops.tune_set("gsw_max_sweeps", ms)
                for sweeps in range(1, 8):
                    x = dev(x0.copy())
                    ops.stencil_gs(dA, x, db, sweeps, direction="backward")
                    got = x.cpu().numpy()
                    assert np.array_equal(got, want[sweeps]), (name, lds, ms, sweeps, np.flatnonzero(got != want[sweeps])[:8])
                ops.stencil_gs_check(dA)
    finally:
        ops.tune_set("gsw_lds", -1)
        ops.tune_set("gsw_max_sweeps", 4)
    # forward and backward share the operator's work buffer: alternating them on one stream stays exact
    x = dev(x0.copy())
    ops.stencil_gs(dA, x, db, 2)
    ops.stencil_gs(dA, x, db, 3, "backward")
    w = x0.copy()
    K.gs_forward(A, w, b, 2)
    oracle_backward(A, w, b, 3)
    assert np.array_equal(x.cpu().numpy(), w)
    ops.stencil_gs_check(dA)


def _full_size(A, sweeps):
    n = A.shape[0]
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack()
    assert ops.stencil_gs_available(dA, "backward") and ops.tune_get("gsw_max_sweeps") == 4
    rng = np.random.default_rng(5)
    x0, b = rng.standard_normal(n), rng.standard_normal(n)
    db = dev(b)
    for direction in ("backward", "forward"):
        want = x0.copy()
        if direction == "forward":
            K.lib().orc_csr_gs_forward(n, A.indptr, A.indices, A.data, want, b, sweeps)
        else:
            oracle_backward(A, want, b, sweeps)
        x = dev(x0.copy())
        ops.stencil_gs(dA, x, db, sweeps, direction)           # one pipelined MULTI launch
        ops.stencil_gs_check(dA)
        got = x.cpu().numpy()
        assert np.array_equal(got, want), (direction, np.flatnonzero(got != want)[:8])


def test_full_size_4097_five_point_three_sweeps_both_directions():
    """cfg#4's fine level (4097^2): 3 sweeps in one launch, backward and forward, bitwise against the oracle."""
    _full_size(K.as_csr(P.poisson_2d_structured(4096)[0]), 3)


def test_full_size_2049_galerkin_three_sweeps_both_directions():
    """Level 1 of cfg#4 (R A P at 2049^2, 9-point): 3 sweeps in one launch, backward and forward, bitwise."""
    A0 = P.poisson_2d_structured(4096)[0]
    Pm = P.geometric_hierarchy_2d(4097, 6)[0]
    A1 = sp.csr_matrix(Pm.T.tocsr() @ A0 @ Pm)
    A1.sort_indices()
    _full_size(K.as_csr(A1), 3)


def _learned_q_level():
    A = P.jittered_poisson_2d(100, seed=42)[0]
    l2 = P.pseudo_l2_interpolator_1d(101)
    Q = P.learned_like(sp.kron(l2, l2).tocsr(), 43)
    Ac = sp.csr_matrix(Q.T @ A @ Q)
    Ac.sort_indices()
    return K.as_csr(Ac)


FALLBACK = {
    "ragged_5pt": lambda: K.as_csr(sp.csr_matrix(grid_operator(203, 77)[: 77 * 203 - 5][:, : 77 * 203 - 5])),
    "jittered_7pt": lambda: K.as_csr(P.jittered_poisson_2d(150, seed=42)[0]),
    "learned_q_galerkin": _learned_q_level,
    "chain_1d": lambda: K.as_csr(P.poisson_1d_fd(3000)[0]),
    "ell_513": lambda: K.as_csr(P.poisson_2d_structured(512)[0]),
}


@pytest.mark.parametrize("name", sorted(FALLBACK))
def test_backward_fallback_schedules_bit_exact(name):
    """Everything the mirrored kernels do not take runs the forward level schedule in reverse (per-set launches, the
    one-workgroup ELL executor, the chain kernel): the same bits as the oracle's rows n-1 .. 0, also through the torch op."""
    A = FALLBACK[name]()
    n = A.shape[0]
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack()
    if name != "ell_513":                                      # (a grid: the schedule is driven directly below)
        assert not ops.stencil_gs_available(dA, "backward"), name
    if name == "ragged_5pt":
        assert ops.stencil_gs_available(dA) and n % dA.stencil.W != 0
        with pytest.raises(LmgError):
            ops.stencil_gs(dA, dev(np.zeros(n)), dev(np.ones(n)), 1, "backward")
    sched = ops.build_gs_schedule(A, "lexicographic", DEV, reverse=True)
    ops.gs_prepare(dA, sched)
    if name == "ell_513":
        assert sched.ell is not None and sched.ell[1] == 5
    if name == "chain_1d":
        assert int(sched.h_ptr[-1]) <= 4 * sched.nsets
    rng = np.random.default_rng(23)
    x0, b = rng.standard_normal(n), rng.standard_normal(n)
    want = oracle_backward(A, x0.copy(), b, 3)
    x = dev(x0.copy())
    ops.csr_gs_schedule(dA, x, dev(b), sched, 3)
    assert np.array_equal(x.cpu().numpy(), want), name
    ops.register_torch_ops()
    h = torch.ops.lmg.operator_create(dev(A.indptr), dev(A.indices), dev(A.data), n)
    try:
        x2 = dev(x0.copy())
        torch.ops.lmg.operator_gauss_seidel_backward_(h, x2, dev(b), 3)
        assert np.array_equal(x2.cpu().numpy(), want), name
    finally:
        torch.ops.lmg.operator_free(h)


def test_torch_op_backward_on_a_grid_operator():
    A = grid_operator(130, 70)
    n = A.shape[0]
    ops.register_torch_ops()
    h = torch.ops.lmg.operator_create(dev(A.indptr), dev(A.indices), dev(A.data), n)
    try:
        assert torch.ops.lmg.operator_format(h) == "stencil"
        rng = np.random.default_rng(3)
        x0, b = rng.standard_normal(n), rng.standard_normal(n)
        x = dev(x0.copy())
        torch.ops.lmg.operator_gauss_seidel_backward_(h, x, dev(b), 5)
        assert np.array_equal(x.cpu().numpy(), oracle_backward(A, x0.copy(), b, 5))
    finally:
        torch.ops.lmg.operator_free(h)


@pytest.mark.parametrize("name", ["poisson2d_513", "ragged_like_jittered"])
def test_backward_multicolor_is_the_colours_in_reverse(name):
    A = K.as_csr(P.poisson_2d_structured(512)[0]) if name == "poisson2d_513" else K.as_csr(P.jittered_poisson_2d(80)[0])
    n = A.shape[0]
    fwd = ops.build_gs_schedule(A, "multicolor", DEV)
    rev = ops.build_gs_schedule(A, "multicolor", DEV, reverse=True)
    rows, ptr = fwd.d_rows.cpu().numpy(), fwd.h_ptr
    order = np.concatenate([rows[ptr[s]:ptr[s + 1]] for s in range(fwd.nsets - 1, -1, -1)]).astype(np.int32)
    rng = np.random.default_rng(9)
    x0, b = rng.standard_normal(n), rng.standard_normal(n)
    want = x0.copy()
    for _ in range(2):
        K.gs_rows(A, want, b, order)
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    x = dev(x0.copy())
    ops.csr_gs_schedule(dA, x, dev(b), rev, 2)
    assert np.array_equal(x.cpu().numpy(), want)


# ---- solvers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweep", ["forward", "backward", "symmetric"])
@pytest.mark.parametrize("name", ["grid_101", "jittered_60"])
def test_gauss_seidel_solver_sweep_directions(sweep, name):
    """GaussSeidel.solve(sweep=...) against an oracle restatement (pyamg semantics: symmetric = forward, then backward)."""
    from learnmultigrid_amd.solvers import GaussSeidel
    A, rhs = P.poisson_2d_structured(100) if name == "grid_101" else P.jittered_poisson_2d(60, seed=42)
    A = K.as_csr(A)
    b = np.ascontiguousarray(rhs, dtype=float).ravel()
    g = GaussSeidel(A, rhs.copy())
    g.solve(max_iterations=15, error=1e-30, sweep=sweep)
    if name == "grid_101":
        assert ops.stencil_gs_available(g._device_matrix(), "backward")
    x = np.zeros(A.shape[0])
    want = []
    for _ in range(15):
        want.append(np.linalg.norm(b - A @ x))
        if sweep in ("forward", "symmetric"):
            K.gs_forward(A, x, b, 1)
        if sweep in ("backward", "symmetric"):
            oracle_backward(A, x, b, 1)
    np.testing.assert_allclose(g.get_track_res().ravel(), want, rtol=1e-10, atol=1e-14 * max(want))
    assert np.array_equal(g.get_solution().ravel(), x)          # the sweeps themselves are bitwise
    with pytest.raises(ValueError):
        GaussSeidel(A, rhs.copy()).solve(max_iterations=1, sweep="sideways")


class ForwardBackwardVCycle(V.HoistedVCycle):
    """The oracle's hoisted V-cycle with forward Gauss-Seidel pre-smoothing and BACKWARD post-smoothing."""

    def cycle(self, x, b, smoother="GaussSeidel", steps=3, omega=1.0, l=0):
        x = np.ascontiguousarray(x, dtype=float).reshape(-1).copy()
        b = np.ascontiguousarray(b, dtype=float).reshape(-1)
        K.gs_forward(self.A[l], x, b, steps)
        r, _ = K.residual(self.A[l], x, b)
        rc = K.matvec(self.R[l], r)
        ec = self.lu.solve(rc) if l + 1 == len(self.P) else self.cycle(np.zeros_like(rc), rc, smoother, steps, omega, l + 1)
        x = K.spmv(self.P[l], ec, x, 1.0, 1.0)
        return oracle_backward(self.A[l], x, b, steps)


@pytest.mark.parametrize("m,levels,its", [(512, 3, 6), (4096, 6, 3)], ids=["cfg2", "cfg4"])
def test_multigrid_forward_backward_cycle_matches_the_oracle(m, levels, its):
    from learnmultigrid_amd.solvers import HierarchyMG
    A, rhs = P.poisson_2d_structured(m)
    hier = P.geometric_hierarchy_2d(m + 1, levels)
    kw = dict(levels=levels, smoother="GaussSeidel", smooth_steps=3, max_iterations=its, error=1e-30)
    mg = HierarchyMG(A, rhs.copy(), hier)
    mg.solve(gs_sweep=("forward", "backward"), **kw)
    got = mg.get_track_res().ravel()
    ref = ForwardBackwardVCycle(A, hier)
    b = rhs.ravel()
    x = np.zeros(A.shape[0])
    want = []
    for _ in range(its):
        want.append(np.linalg.norm(b - A @ x))
        x = ref.cycle(x, b, "GaussSeidel", 3)
    want = np.array(want)
    assert got[0] == np.sqrt(float(A.shape[0]))
    np.testing.assert_allclose(got[1:], want[1:], rtol=1e-10, atol=1e-14 * want.max())
    mg2 = HierarchyMG(A, rhs.copy(), hier)
    mg2.solve(gs_sweep=("forward", "backward"), use_graph=True, **kw)
    assert np.array_equal(mg2.get_track_res(), mg.get_track_res())          # hipGraph replay == eager
    assert np.array_equal(mg2.get_solution(), mg.get_solution())
    if m == 512:
        a = HierarchyMG(A, rhs.copy(), hier)
        a.solve(gs_sweep="forward", **kw)
        c = HierarchyMG(A, rhs.copy(), hier)
        c.solve(**kw)
        assert np.array_equal(a.get_track_res(), c.get_track_res())
        assert np.array_equal(a.get_solution(), c.get_solution())
        s = HierarchyMG(A, rhs.copy(), hier)
        s.solve(gs_sweep="symmetric", use_graph=True, **kw)                    # a launch per direction and step
        assert s.get_track_res()[-1, 0] < 1e-3 * s.get_track_res()[1, 0]
        with pytest.raises(ValueError):
            HierarchyMG(A, rhs.copy(), hier).solve(gs_sweep=("forward", "sideways"), **kw)


def _symmetric_problem(m=256):
    A, rhs = P.poisson_2d_structured(m)
    s = m + 1
    idx = np.arange(s * s)
    inter = ((idx % s) > 0) & ((idx % s) < m) & ((idx // s) > 0) & ((idx // s) < m)
    keep = sp.diags(inter.astype(float))
    As = sp.csr_matrix(keep @ A @ keep + sp.diags((~inter).astype(float)))
    return As, rhs, s


def test_forward_backward_vcycle_is_a_symmetric_preconditioner():
    from learnmultigrid_amd.hierarchy import Hierarchy
    from learnmultigrid_amd.solvers import CG
    As, rhs, s = _symmetric_problem()
    H = Hierarchy(As, P.geometric_hierarchy_2d(s, 5), DEV)
    fine = H.levels[0]
    rng = np.random.default_rng(31)
    r1, r2 = rng.standard_normal(As.shape[0]), rng.standard_normal(As.shape[0])

    def M(r, pair):
        fine.b.copy_(dev(r))
        H.cycle("GaussSeidel", 2, 1.0, x_is_zero=True, gs_sweep=pair)
        return fine.x.cpu().numpy().copy()

    def asym(pair):
        m1, m2 = M(r1, pair), M(r2, pair)
        return abs(r1 @ m2 - r2 @ m1) / (np.linalg.norm(r1) * np.linalg.norm(m2))

    assert asym(("forward", "backward")) <= 1e-10
    assert asym(("forward", "forward")) >= 1e-6                 # the check can tell the two apart
    H.check_smoothers()
    plain = CG(As, rhs.copy())
    plain.solve(max_iterations=3000, error=1e-10)
    jac = CG(As, rhs.copy())
    jac.solve(max_iterations=200, error=1e-10, preconditioner=H)
    gs = CG(As, rhs.copy())
    gs.solve(max_iterations=200, error=1e-10, preconditioner=H, precond_smoother="GaussSeidel")
    assert gs.get_track_res()[-1, 0] <= 1e-10
    assert gs.get_iterations() <= jac.get_iterations()
    x_ref = plain.get_solution()
    assert np.linalg.norm(gs.get_solution() - x_ref) <= 1e-6 * np.linalg.norm(x_ref)
    with pytest.raises(ValueError):
        CG(As, rhs.copy()).solve(max_iterations=1, preconditioner=H, precond_smoother="SOR")
