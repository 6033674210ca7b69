"""The K-cycle on the device (-m gpu): the two inner steps (csrc/krylov.hip, lmg_kcycle_step1 / lmg_kcycle_step2) against the
NumPy lines of kcycle_ref -- products within the bar of lmg_dot, everything derived from them bit for bit from the
products read back --, their forms against each other, aliasing, guards and status codes; then whole cycles against the
twin (kcycle_ref.KCycle), through the solver front ends, eager and from a captured graph.

Sizes of the kernel tests: n = 1, 2 (no pair / one pair), 255, 257, 4099 (odd, three shares), the largest n of the
one-launch form and the next one, and 1314819 = 2^20 + 2^18 + 4099: odd, the full grid of 512 shares, every lane beyond
its fourth pair step and some beyond the fifth."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import kcycle_ref as KR                                   # noqa: E402  (checker only)
from learnmultigrid_amd import _lib, ops, problems as P   # noqa: E402
from learnmultigrid_amd._lib import LmgError              # noqa: E402
from cycle_shapes_ref import ShapeCycle, history          # noqa: E402  (checker only)
from support import DEV                                   # noqa: E402

F64 = torch.float64
PAD = 2                                                    # doubles of NaN in front of a vector: its base stays on 16 bytes
FORMS = ("two", "one", "auto")
NAMES = ("c1", "v1", "b", "c2", "v2")
IDX = {name: i for i, name in enumerate(ops.KCYCLE_SCALARS)}


def sizes():
    edge = ops.kcycle_one_launch_max()
    return (1, 2, 255, 257, 4099, edge, edge + 1, (1 << 20) + (1 << 18) + 4099)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def spread(rng, size):
    """Entries over 1e-8 .. 1e+8 with random signs: a summation-order mistake moves the result far beyond the bar."""
    return rng.choice((-1.0, 1.0), size) * 10.0 ** rng.uniform(-8.0, 8.0, size)


def padded(values_or_n):
    """(allocation, view): the vector inside an allocation with NaN on either side."""
    n = values_or_n if isinstance(values_or_n, int) else values_or_n.size
    full = torch.full((n + 2 * PAD,), float("nan"), dtype=F64, device=DEV)
    view = full[PAD:PAD + n]
    if not isinstance(values_or_n, int):
        view.copy_(torch.from_numpy(values_or_n))
    return full, view


def padding_is_nan(full):
    return bool(torch.isnan(full[:PAD]).all()) and bool(torch.isnan(full[-PAD:]).all())


class Case:
    def __init__(self, n, seed=0):
        self.n = n
        rng = np.random.default_rng(7919 * seed + n % 9973)
        self.host = {name: spread(rng, n) for name in NAMES}
        self.upload()

    def upload(self):
        self.full, self.dev = {}, {}
        for name in NAMES:
            self.full[name], self.dev[name] = padded(self.host[name])
        self.before = {name: self.full[name].clone() for name in NAMES}

    def inputs_untouched(self):
        # (NaN padding included: equal bit patterns)
        return all(torch.equal(self.full[k].view(torch.int64), self.before[k].view(torch.int64)) for k in NAMES)

    def scratch(self):
        return (torch.full((len(ops.KCYCLE_SCALARS),), float("nan"), dtype=F64, device=DEV),
                torch.full((ops.kcycle_partials_count(self.n),), 123.0, dtype=F64, device=DEV))

    def step1(self, k_inner, form):
        d = self.dev
        rt_full, rt = padded(self.n)
        scal, part = self.scratch()
        ops.kcycle_step1(k_inner, d["c1"], d["v1"], d["b"], rt, scal, part, form=form)
        assert padding_is_nan(rt_full) and bool(torch.isnan(scal[3:]).all())
        return rt, scal

    def step2(self, k_inner, form, rt, scal1, alias=False):
        d = self.dev
        scal, part = self.scratch()
        scal[:3] = scal1[:3]
        if alias:
            x_full, x = padded(self.host["c2"])
            c2 = x
        else:
            (x_full, x), c2 = padded(self.n), d["c2"]
        ops.kcycle_step2(k_inner, d["c1"], d["v1"], c2, d["v2"], rt, scal, x, part, form=form)
        assert padding_is_nan(x_full)
        return x, scal


def within_bar(got, p, q, what):
    want, bar = float(p @ q), 1e-13 * float(np.abs(p) @ np.abs(q))
    print("%s: |got - want| / (|p| . |q|) = %.3e" % (what, abs(got - want) / max(bar / 1e-13, 1e-300)))
    assert np.isfinite(got) and abs(got - want) <= bar, (what, got, want, bar)


@pytest.fixture(scope="module", params=range(8), ids=lambda i: "size%d" % i)
def case(request):
    return Case(sizes()[request.param])


def test_geometry():
    edge = ops.kcycle_one_launch_max()
    assert edge >= 1024 and edge & (edge - 1) == 0
    assert [ops.kcycle_grid(n) for n in (1, 2048, 2049, 1 << 20, 1 << 24)] == [1, 1, 2, 512, 512]
    assert ops.kcycle_partials_count(1 << 24) == 3 * 512
    assert tuple(ops.KCYCLE_SCALARS) == KR.SCALARS


@pytest.mark.parametrize("k_inner", KR.K_INNER)
def test_both_steps(case, k_inner):
    n, h = case.n, case.host
    # ---- step 1
    rt, scal = case.step1(k_inner, "two")
    s = scal.cpu().numpy()
    p1 = KR.direction(k_inner, h["c1"], h["v1"])
    within_bar(s[IDX["alpha1"]], p1, h["b"], "n %d %s alpha1" % (n, k_inner))
    within_bar(s[IDX["rho1"]], p1, h["v1"], "n %d %s rho1" % (n, k_inner))
    t1 = KR.step1_coefficients(s[IDX["alpha1"]], s[IDX["rho1"]])
    assert same_bits(s[IDX["t1"]], t1)
    rt_host = rt.cpu().numpy()
    assert same_bits(rt_host, KR.step1_vector(h["b"], h["v1"], t1))
    for form in FORMS + ("two",):                                  # every form, and a second call of the first
        rt_f, scal_f = case.step1(k_inner, form)
        assert same_bits(rt_f.cpu().numpy(), rt_host) and same_bits(scal_f[:3].cpu().numpy(), s[:3]), form
    # ---- step 2
    x, scal2 = case.step2(k_inner, "two", rt, scal)
    s2 = scal2.cpu().numpy()
    assert same_bits(s2[:3], s[:3])
    p2 = KR.direction(k_inner, h["c2"], h["v2"])
    within_bar(s2[IDX["gamma"]], p2, h["v1"], "n %d %s gamma" % (n, k_inner))
    within_bar(s2[IDX["beta"]], p2, h["v2"], "n %d %s beta" % (n, k_inner))
    within_bar(s2[IDX["alpha2"]], p2, rt_host, "n %d %s alpha2" % (n, k_inner))
    rho2, t2, a = KR.step2_coefficients(s2[IDX["rho1"]], s2[IDX["t1"]], s2[IDX["gamma"]], s2[IDX["beta"]], s2[IDX["alpha2"]])
    assert same_bits([s2[IDX["rho2"]], s2[IDX["t2"]], s2[IDX["a"]]], [rho2, t2, a])
    x_host = x.cpu().numpy()
    assert same_bits(x_host, KR.step2_vector(h["c1"], h["c2"], a, t2))
    for form in FORMS + ("two",):
        for alias in (False, True):
            x_f, scal_f = case.step2(k_inner, form, rt, scal, alias=alias)
            assert same_bits(x_f.cpu().numpy(), x_host) and same_bits(scal_f.cpu().numpy(), s2), (form, alias)
    assert case.inputs_untouched() and same_bits(rt.cpu().numpy(), rt_host)


@pytest.mark.parametrize("n", [257, 4099])
@pytest.mark.parametrize("k_inner", KR.K_INNER)
def test_guards(n, k_inner):
    c = Case(n, seed=1)
    # p1 = 0: t1 = 0 and rt is b
    c.host["v1" if k_inner == "gcr" else "c1"] = np.zeros(n)
    c.upload()
    for form in FORMS:
        rt, scal = c.step1(k_inner, form)
        s = scal.cpu().numpy()
        assert s[IDX["rho1"]] == 0.0 and s[IDX["t1"]] == 0.0 and same_bits(rt.cpu().numpy(), c.host["b"]), form
    # the second direction parallel to the first: rho2 = 0, t2 = 0, x = t1 c1
    c = Case(n, seed=2)
    c.host["c2"], c.host["v2"] = 2.0 * c.host["c1"], 2.0 * c.host["v1"]
    c.upload()
    for form in FORMS:
        rt, scal = c.step1(k_inner, form)
        x, scal2 = c.step2(k_inner, form, rt, scal)
        s2 = scal2.cpu().numpy()
        assert s2[IDX["rho2"]] == 0.0 and s2[IDX["t2"]] == 0.0 and same_bits(s2[IDX["a"]], s2[IDX["t1"]]), form
        assert s2[IDX["t1"]] != 0.0 and same_bits(x.cpu().numpy(), s2[IDX["t1"]] * c.host["c1"]), form


def test_status_codes():
    n = 4099
    c = Case(n, seed=3)
    L, d = _lib.lib(), c.dev
    rt_full, rt = padded(n)
    x_full, x = padded(n)
    scal, part = c.scratch()
    p = lambda t: t.data_ptr()                                                           # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    np_ = part.numel()

    def s1(n=n, gcr=1, form=0, c1=p(d["c1"]), v1=p(d["v1"]), b=p(d["b"]), rt=p(rt), scal=p(scal), part=p(part), count=np_):
        return L.lmg_kcycle_step1(n, gcr, form, c1, v1, b, rt, scal, part, count, st)

    def s2(n=n, gcr=1, form=0, c1=p(d["c1"]), v1=p(d["v1"]), c2=p(d["c2"]), v2=p(d["v2"]), rt=p(d["b"]), scal=p(scal),
           x=p(x), part=p(part), count=np_):
        return L.lmg_kcycle_step2(n, gcr, form, c1, v1, c2, v2, rt, scal, x, part, count, st)

    ARG, ALIGN = -1, -2
    for call, names in ((s1, ("c1", "v1", "b", "rt", "scal", "part")), (s2, ("c1", "v1", "c2", "v2", "rt", "scal", "x", "part"))):
        for name in names:
            assert call(**{name: None}) == ARG, name
            if name not in ("scal", "part"):
                assert call(**{name: p(d["c1"]) + 8 if name == "c1" else p(d["v2"]) + 8}) == ALIGN, name
        assert call(n=0) == ARG and call(n=-5) == ARG
        assert call(form=3) == ARG and call(form=-1) == ARG
        assert call(count=np_ - 1) == ARG and call(count=0) == ARG
    for name in ("c1", "v1", "b"):
        assert s1(rt=p(d[name])) == ARG, name
    for name in ("c1", "v1", "v2", "b"):                                                 # (b stands in for rt here)
        assert s2(x=p(d[name])) == ARG, name
    torch.cuda.synchronize()
    assert bool(torch.isnan(rt_full).all()) and bool(torch.isnan(x_full).all()) and bool(torch.isnan(scal).all())
    assert c.inputs_untouched()
    with pytest.raises(ValueError):
        ops.kcycle_step1("cg", d["c1"], d["v1"], d["b"], rt, scal, part)
    with pytest.raises(ValueError):
        ops.kcycle_step1("gcr", d["c1"], d["v1"], d["b"], rt, scal, part, form="three")
    with pytest.raises(LmgError):
        ops.kcycle_step1("gcr", d["c1"], d["v1"], d["b"], rt, scal, part[:-1])


# ---- cycles -----------------------------------------------------------------------------------------------------------------
JAC = dict(smoother="Jacobi", smoother_semantics="as_named", omega=0.8)
GS = dict(smoother="Jacobi")                                  # as shipped: forward Gauss-Seidel whatever the name
ITS = 3


def _compare(mg, A, rhs, hier, k_inner, **kw):
    want, xw = history(KR.KCycle(A, hier, k_inner), A, rhs, ITS, **kw)
    got = mg.get_track_res().ravel()
    assert got.shape == want.shape and got[0] == np.sqrt(float(A.shape[0]))
    np.testing.assert_allclose(got[1:], want[1:], rtol=1e-10, atol=1e-14 * want.max())
    np.testing.assert_allclose(mg.get_solution().ravel(), xw, rtol=1e-10, atol=1e-12 * np.abs(xw).max())


def _bitwise(a, b):
    assert np.array_equal(a.get_track_res(), b.get_track_res())
    assert np.array_equal(a.get_solution(), b.get_solution())


def _solve(mg, levels, k_inner, graph=False, **kw):
    mg.solve(levels=levels, smooth_steps=2, max_iterations=ITS, error=1e-30, cycle_shape="K", k_inner=k_inner,
             use_graph=graph, **kw)
    return mg


@pytest.mark.parametrize("k_inner", KR.K_INNER)
@pytest.mark.parametrize("smoothing,twin", [(JAC, dict(smoother="Jacobi", steps=2, omega=0.8)), (GS, dict(smoother="GaussSeidel", steps=2))],
                         ids=["jacobi", "gauss_seidel"])
def test_geometric_cycles(smoothing, twin, k_inner):
    """65^2, 4 levels: the levels below the finest run the fused tiled passes around the two inner steps."""
    from learnmultigrid_amd.solvers import HierarchyMG
    m, levels = 64, 4
    A, rhs = P.poisson_2d_structured(m)
    hier = P.geometric_hierarchy_2d(m + 1, levels)
    mg = _solve(HierarchyMG(A, rhs.copy(), hier), levels, k_inner, **smoothing)
    _compare(mg, A, rhs, hier, k_inner, **twin)
    H = mg._hier
    assert H.kscal is not None and all(lev.kc is not None for lev in H.levels[1:-1])
    replayed = _solve(HierarchyMG(A, rhs.copy(), hier), levels, k_inner, graph=True, **smoothing)    # (replays ITS times)
    _bitwise(mg, replayed)
    assert [k[5:7] for k in replayed._hier._graphs] == [("K", k_inner)]
    w = HierarchyMG(A, rhs.copy(), hier)
    w.solve(levels=levels, smooth_steps=2, max_iterations=ITS, error=1e-30, cycle_shape="W", **smoothing)
    assert not np.array_equal(w.get_track_res(), mg.get_track_res())


def test_k_cycle_method_and_keywords():
    from learnmultigrid_amd.solvers import HierarchyMG
    m, levels = 64, 4
    A, rhs = P.poisson_2d_structured(m)
    hier = P.geometric_hierarchy_2d(m + 1, levels)
    mg = HierarchyMG(A, rhs.copy(), hier)
    u = np.random.default_rng(3).standard_normal((A.shape[0], 1))
    for k_inner in KR.K_INNER:
        out = mg.k_cycle(A, u.copy(), rhs, "Jacobi", 2, 1e-8, levels, smoother_semantics="as_named", omega=0.8, k_inner=k_inner)
        want = KR.KCycle(A, hier, k_inner).cycle(u.ravel(), rhs.ravel(), "Jacobi", 2, 0.8)
        np.testing.assert_allclose(out.ravel(), want, rtol=1e-10, atol=1e-12 * np.abs(want).max())
    for bad in (dict(cycle_shape="k"), dict(cycle_shape="KK"), dict(cycle_shape=None), dict(cycle_shape="K", k_inner="cg")):
        with pytest.raises(ValueError):
            mg.solve(levels=levels, **bad)
    with pytest.raises(ValueError, match="solve_many has no 'K' cycle"):
        mg.solve_many(np.tile(rhs, (1, 2)), levels=levels, cycle_shape="K")
    # two levels: the V-cycle, bit for bit
    two = P.geometric_hierarchy_2d(m + 1, 2)
    k2 = _solve(HierarchyMG(A, rhs.copy(), two), 2, "gcr", **JAC)
    v2 = HierarchyMG(A, rhs.copy(), two)
    v2.solve(levels=2, smooth_steps=2, max_iterations=ITS, error=1e-30, cycle_shape="V", **JAC)
    _bitwise(k2, v2)


@pytest.mark.parametrize("smoothing,twin", [(JAC, dict(smoother="Jacobi", steps=2, omega=0.8)), (GS, dict(smoother="GaussSeidel", steps=2))],
                         ids=["jacobi", "gauss_seidel"])
def test_classical_amg_cycles(smoothing, twin):
    """33^2 with PMIS levels down to at most 30 rows: sliced-ELL operators, no grid twins."""
    from learnmultigrid_amd.solvers import ClassicalAMG
    A, rhs = P.poisson_2d_structured(32)
    mg = _solve(ClassicalAMG(A, rhs.copy(), max_coarse=30), None, "gcr", **smoothing)
    H = mg._hier
    assert len(H.levels) >= 3
    hier = [lev.P.to_scipy() for lev in H.levels[:-1]]
    _compare(mg, A, rhs, hier, "gcr", **twin)
    _bitwise(mg, _solve(ClassicalAMG(A, rhs.copy(), max_coarse=30), None, "gcr", graph=True, **smoothing))


@pytest.mark.parametrize("smoothing,twin", [(JAC, dict(smoother="Jacobi", steps=2, omega=0.8)), (GS, dict(smoother="GaussSeidel", steps=2))],
                         ids=["jacobi", "gauss_seidel"])
def test_aggregation_cycles(smoothing, twin):
    from learnmultigrid_amd.solvers import HierarchyMG
    A, rhs = P.poisson_2d_structured(80)
    hier = KR.aggregation_hierarchy(81, 4)
    for k_inner in KR.K_INNER:
        mg = _solve(HierarchyMG(A, rhs.copy(), hier), 4, k_inner, **smoothing)
        _compare(mg, A, rhs, hier, k_inner, **twin)
        _bitwise(mg, _solve(HierarchyMG(A, rhs.copy(), hier), 4, k_inner, graph=True, **smoothing))


def test_fp32_cycle_operators_precondition_with_k_cycles():
    """A hierarchy with cycle_values="f32" runs K-cycles as a GMRES preconditioner; its inner products use the rounded operator.
    The operators of the cycle move by 2^-24 relatively, far below what the cycle leaves of an error, so the iteration count to
    1e-8 |b| is that of the fp64 hierarchy give or take a step across the threshold: at most two more are accepted."""
    from learnmultigrid_amd.hierarchy import Hierarchy
    from learnmultigrid_amd.solvers import GMRES
    A, rhs = P.poisson_2d_structured(80)
    hier = KR.aggregation_hierarchy(81, 4)
    tol = 1e-8 * float(np.linalg.norm(rhs))
    its = {}
    for values in ("f64", "f32"):
        H = Hierarchy(A, hier, DEV, cycle_values=values)
        gm = GMRES(A, rhs.copy())
        gm.solve(max_iterations=100, error=tol, restart=10, preconditioner=H, precond_steps=2, precond_omega=0.8,
                 precond_cycle_shape="K")
        x = gm.get_solution().ravel()
        assert gm.get_track_res()[-1, 0] <= tol and np.linalg.norm(rhs.ravel() - A @ x) <= 1.0001 * tol, values
        its[values] = gm.iterations
    print("GMRES(10) + K(2,2) iterations, 81^2 aggregation: fp64 operators %d, fp32 operators %d" % (its["f64"], its["f32"]))
    assert its["f32"] <= its["f64"] + 2


def test_gmres_with_k_cycles_on_aggressive_aggregation():
    """243^2, 5 levels of 3 x 3 aggregation, GMRES(10) + V(2,2)-shaped cycles, damped Jacobi, to 1e-8 |b|."""
    from learnmultigrid_amd.hierarchy import Hierarchy
    from learnmultigrid_amd.solvers import GMRES
    A, rhs = P.poisson_2d_structured(242)
    H = Hierarchy(A, KR.aggregation_hierarchy(243, 5), DEV)
    tol = 1e-8 * float(np.linalg.norm(rhs))

    def iterations(shape, **kw):
        gm = GMRES(A, rhs.copy())
        gm.solve(max_iterations=200, error=tol, restart=10, preconditioner=H, precond_steps=2, precond_omega=0.8,
                 precond_cycle_shape=shape, **kw)
        assert gm.get_track_res()[-1, 0] <= tol, shape
        x = gm.get_solution().ravel()
        assert np.linalg.norm(rhs.ravel() - A @ x) <= 1.0001 * tol
        return gm.iterations

    its_v, its_w = iterations("V"), iterations("W")
    for k_inner in KR.K_INNER:
        its_k = iterations("K", precond_k_inner=k_inner)
        print("GMRES(10) iterations: V %d, W %d, K(%s) %d" % (its_v, its_w, k_inner, its_k))
        assert its_k < its_w < its_v and 2 * its_k <= its_v, (k_inner, its_k, its_w, its_v)
    with pytest.raises(ValueError):
        GMRES(A, rhs.copy()).solve(preconditioner=H, precond_cycle_shape="K", precond_k_inner="cg")
    with pytest.raises(ValueError, match="solve_many has no 'K' cycle"):
        GMRES(A, rhs.copy()).solve_many(np.tile(rhs, (1, 2)), preconditioner=H, precond_cycle_shape="K")
