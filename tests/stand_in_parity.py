"""TEST-ONLY: what every CPU stand-in of learnmultigrid_amd.ops is compared with its kernel on (no kernel reads this file;
importing it needs no GPU).

REGISTRY has one entry per name that a stand-in namespace offers (NAMESPACES: cpu_ops_shim and its factories, the block
namespaces of block_cg_ref, block_gmres_ref and test_block_cpu, line_band_ref.stand_in()).  An entry is one of

    Cases       small input builders and the comparison rule of the op; tests/test_stand_in_parity_gpu.py runs each of them
                through the stand-in on CPU tensors and through ops on device copies and compares EVERY tensor argument
    CoveredBy   the id of a GPU test that already runs this stand-in and the kernel on the same inputs
    NoValues    a size helper, a test knob or a re-export: one line says why there is nothing to compare

tests/test_shim_signatures_cpu.py fails when a namespace offers a function or class without an entry.

How a case runs (Side).  The inputs are built once on the host.  A tensor the op does not write (ro) must hold the bits that
went in afterwards, on both sides.  A tensor the op writes (rw) is the head of an allocation GUARD elements longer whose tail
holds SENTINEL and must keep it (sweep_variants.Guarded, and the same layout on the CPU); where the op must not read it, it
starts as NaN.  Scratch (the partials of a reduction) is the one kind of argument that is not compared: its contents are the
kernel's own business.  Results are compared bit for bit unless the case names a bound for them.

The bound.  Where the two sides add the same m products in different orders, each computed sum is within gamma_m sum|terms|
of the exact one (gamma_m = m u / (1 - m u), u = 2^-53; Higham, Accuracy and Stability, 3.1), so they differ by at most
2 gamma_m sum|terms| -- the argument of nmg2d_cases.product_bound.  Quantities computed from such a sum inherit the bound;
the derivation stands next to the case.  No bound is fitted to an observed difference."""
import functools
import inspect

import numpy as np
import scipy.sparse as sp
import torch

import block_cg_ref
import block_gmres_ref
import chebyshev_ref as CR
import cpu_ops_shim as shim
import line_band_ref as LB
from learnmultigrid_amd import problems as P
from learnmultigrid_amd.ops import DeviceCSR
from oracle import kernels as K
from support import operators
from sweep_variants import ALPHA_BETA, GUARD, SENTINEL, Guarded, sell_problem

F64 = torch.float64
U = 2.0 ** -53
WIDTHS = (2, 4, 8)
SECOND_TRIP = 262144 + 257      # the smallest n at which a lane of the 1024 x 256 geometry makes a second trip


def gamma(m):
    return m * U / (1.0 - m * U)


def _test_block_cpu_namespace():
    import test_block_cpu
    return test_block_cpu.block_namespace()


NAMESPACES = {
    "module": lambda: shim,
    "namespace": shim.namespace,
    "recording_line": shim.recording_line,
    "fused_jacobi": lambda: shim.fused("jacobi"),
    "fused_cheby": lambda: shim.fused("cheby"),
    "fused_all": lambda: shim.fused("all"),
    "block_cg": lambda: block_cg_ref.block_namespace(shim),
    "block_gmres": lambda: block_gmres_ref.block_namespace(shim),
    "line_band": LB.stand_in,
    "test_block_cpu": _test_block_cpu_namespace,
}


def offered(ns):
    """The functions and classes a namespace offers under a public name (the factories of cpu_ops_shim are its own tools)."""
    return {k: v for k, v in vars(ns).items()
            if not k.startswith("_") and k not in shim.FACTORIES and (inspect.isfunction(v) or inspect.isclass(v))}


def all_offered():
    """name -> the namespaces that offer it."""
    out = {}
    for nsname, make in NAMESPACES.items():
        for k in offered(make()):
            out.setdefault(k, []).append(nsname)
    return out


def implementations(op, only=None):
    """[(namespace name, namespace)]: one namespace per distinct function that stands for `op` (a copy of the module's own
    function counts once; a recording wrapper is a function of its own)."""
    seen, out = [], []
    for nsname, make in NAMESPACES.items():
        if only is not None and nsname not in only:
            continue
        ns = make()
        fn = vars(ns).get(op)
        if fn is None or any(fn is f for f in seen):
            continue
        seen.append(fn)
        out.append((nsname, ns))
    return out


# ---- the two sides of a case ------------------------------------------------------------------------------------------------
class Refused(Exception):
    """The real predicate of a fused pass refuses the shape: the one reason for which a case may be skipped."""


class HostGuarded(Guarded):
    """sweep_variants.Guarded's layout on CPU tensors."""

    def __init__(self, n, fill):
        self.n = n
        self.buf = torch.full((n + GUARD,), SENTINEL, dtype=F64)
        self.out = self.buf[:n]
        self.out.copy_(torch.from_numpy(np.ascontiguousarray(fill)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float64:
        return a == b
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


class Side:
    """One side of a case: the ops module (the real one on DEV, a stand-in namespace on "cpu") and every tensor the case
    hands to it, by name."""

    def __init__(self, ops_mod, device):
        self.ops, self.device = ops_mod, device
        self.on_device = device != "cpu"
        self._ro, self._rw, self._mats, self._kept = {}, {}, {}, {}

    def ro(self, name, a):
        """A tensor the op must not write."""
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.copy()).to(self.device)
        self._ro[name] = (t, a)
        return t

    def rw(self, name, init):
        """A tensor the op writes, with the guarded tail; init: its contents (NaN where the op must not read)."""
        init = np.array(init, dtype=np.float64, order="C")           # (a copy: the inputs stay as they were built)
        g = (Guarded if self.on_device else HostGuarded)(init.size, init.reshape(-1))
        self._rw[name] = (g, init.shape)
        return g.out.view(init.shape)

    def scratch(self, count):
        """Partials of a reduction: not compared."""
        return torch.full((max(int(count), 1),), np.nan, dtype=F64, device=self.device)

    def csr(self, name, A, canonical=True, pack=False):
        """The matrix as a DeviceCSR of this side (canonical=False: the arrays as they are, in storage order); pack: with
        the twins pack() chooses (on the CPU pack() builds none)."""
        A = sp.csr_matrix(A)
        H = sp.csr_matrix((A.data.copy(), A.indices.copy(), A.indptr.copy()), shape=A.shape)
        M = DeviceCSR.from_scipy(H, self.device, canonical=canonical)
        if pack:
            M.pack()
        self._mats[name] = (M, M.rowptr.clone(), M.colidx.clone(), M.vals.clone())
        return M

    def keep(self, name, value):
        """A result the op returns (a tensor, an array or a number): compared like a written tensor."""
        self._kept[name] = value

    def require(self, ok, why):
        if self.on_device and not ok:
            raise Refused(why)

    def results(self, tag):
        """name -> host array of everything written or returned; asserts that the inputs and the guards are intact."""
        for name, (t, a) in self._ro.items():
            assert same_bits(t.cpu().numpy(), a).all(), (tag, name, "an input was written")
        for name, (M, rp, ci, va) in self._mats.items():
            assert torch.equal(M.rowptr, rp) and torch.equal(M.colidx, ci), (tag, name, "the pattern of an input was written")
            assert same_bits(M.vals.cpu().numpy(), va.cpu().numpy()).all(), (tag, name, "the values of an input were written")
        out = {}
        for name, (g, shape) in self._rw.items():
            out[name] = g.result((tag, name)).reshape(shape).copy()
        for name, v in self._kept.items():
            out[name] = np.array(v.detach().cpu().numpy() if torch.is_tensor(v) else v)
        return out


def compare(tag, got, want, bounds):
    """Every result of the device side against the stand-in's: bit for bit, or within bounds[name] where one is given.
    Returns {name: largest error / bound} of the bounded ones."""
    assert sorted(got) == sorted(want), (tag, sorted(got), sorted(want))
    worst = {}
    for name, w in want.items():
        g = got[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, name, g.shape, w.shape, g.dtype, w.dtype)
        if name not in bounds:
            eq = same_bits(g, w)
            assert eq.all(), (tag, name, "first differences at", np.flatnonzero(~eq.reshape(-1))[:8],
                              g.reshape(-1)[~eq.reshape(-1)][:4], w.reshape(-1)[~eq.reshape(-1)][:4])
            continue
        b = np.broadcast_to(np.asarray(bounds[name], dtype=np.float64), w.shape)
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (tag, name, "NaN in other places")
        err, bb = np.abs(g - w)[~nan], b[~nan]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bb)
        worst[name] = float(ratio.max()) if ratio.size else 0.0
        assert (err <= bb).all(), (tag, name, "largest error / bound", worst[name])
    return worst


# ---- registry ------------------------------------------------------------------------------------------------------------------
class Case:
    """label: the case's name inside its op.  inputs(): the host arrays, built once.  run(side, inputs): hands them to
    side.ops.  bounds(inputs): {result name: bound} of the results that are not compared bit for bit.  post(inputs,
    results): further assertions on one side's results.  raises: the exception both sides must raise instead."""

    def __init__(self, label, inputs, run, bounds=None, post=None, raises=None):
        self.label, self.run, self.bounds, self.post, self.raises = label, run, bounds, post, raises
        self.inputs = functools.lru_cache(maxsize=None)(inputs)


class Cases:
    def __init__(self, cases, deviation=None, only=None):
        self.cases, self.deviation, self.only = list(cases), deviation, only


class CoveredBy:
    def __init__(self, test_id):
        self.test_id = test_id                       # "<file under tests/>::<test function>"


class NoValues:
    def __init__(self, reason):
        self.reason = reason


REGISTRY = {}


def rng(*key):
    return np.random.default_rng([20240, *key])


# ---- matrices ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def local_block():
    """The local operators of rank 1 of 3 on the 17 x 17 five-point operator, two levels, a halo of two layers (the inner one
    carries real rows, the outer one is empty): cut by the setup steps of dist.DistributedVCycle themselves, in the order its
    constructor runs them, on CPU tensors.  The two collectives of the setup are left out -- what they agree on only enters
    the send lists of the exchange plan, which no kernel reads -- so no process group is needed.
    Returns (A (n_tot x n_tot), R (owned coarse rows x n_tot), P (n_tot x coarse rows)) as SciPy matrices in storage order."""
    from learnmultigrid_amd.dist import DistributedVCycle
    from learnmultigrid_amd.hierarchy import Hierarchy
    m = 16
    A, _ = P.poisson_2d_structured(m)
    D = object.__new__(DistributedVCycle)
    D.ops, D.device, D.group, D.world, D.rank, D.halo_depth = shim, torch.device("cpu"), None, 3, 1, 2
    D.full = Hierarchy(A, P.geometric_hierarchy_2d(m + 1, 2), "cpu", ops_mod=shim)
    D.n_dist = D._choose_distributed_levels(100)
    D.bounds, D.grid_side = D._row_bounds(m + 1)
    assert D.n_dist == 1 and D.grid_side == m + 1
    s = D._ghost_layers(0, None)
    D.dl = [D._make_level(0, s.ghosts, [np.zeros(0, dtype=np.int64)] * D.world)]
    D._cut_local_operators(0, s)
    d = D.dl[0]
    assert d.n_lo > m + 1 and d.n_hi > m + 1 and d.A.shape == (d.n_tot, d.n_tot) and d.R.shape[0] < d.R.shape[1] == d.n_tot
    empty = np.diff(d.A.rowptr.numpy()) == 0
    ghost = np.ones(d.n_tot, dtype=bool)
    ghost[d.own] = False
    assert not empty[~ghost].any() and empty[ghost].any() and not empty[ghost].all()     # real and empty ghost rows
    return tuple(sp.csr_matrix((M.vals.numpy().copy(), M.colidx.numpy().copy(), M.rowptr.numpy().copy()), shape=M.shape)
                 for M in (d.A, d.R, d.P))


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "33":                                  # the 33 x 33 five-point operator, 1089 rows: several workgroups, odd
        return K.as_csr(P.poisson_2d_structured(32)[0])
    if name == "33_permuted":                         # test_torch_ops_gpu._operator("33_permuted")
        A = matrix("33")
        p = np.random.default_rng(11).permutation(A.shape[0])
        return K.as_csr(A[p][:, p])
    if name == "ragged":                              # 321 rows, empty rows, rows without a diagonal, random values
        return sell_problem("ragged_slices").A
    if name == "33_dupdiag":
        # the 33 x 33 operator with its values scaled at random, and in every third row a SECOND diagonal entry of the
        # other sign behind the last entry: not sorted, not duplicate-free, and |a| + |b| != |a + b|
        A = matrix("33")
        r = rng(7)
        rp, ci, va = [0], [], []
        for i in range(A.shape[0]):
            s, e = A.indptr[i], A.indptr[i + 1]
            ci.extend(A.indices[s:e])
            va.extend(A.data[s:e] * r.uniform(0.5, 1.5, e - s))
            if i % 3 == 0:
                ci.append(i)
                va.append(-0.25 * abs(A[i, i]) * r.uniform(0.5, 1.5))
            rp.append(len(ci))
        M = sp.csr_matrix((np.array(va), np.array(ci, dtype=np.int32), np.array(rp, dtype=np.int32)), shape=A.shape)
        assert M.nnz == A.nnz + 363 and not M.has_canonical_format
        return M
    if name == "ragged_top":
        # the first 200 rows of the ragged matrix over all 321 columns: a rectangular block [owned | ghosts] whose diagonal
        # is column == row, swept with x, b and the output over all 321 slots -- the kernel writes the first 200 only
        return K.as_csr(matrix("ragged")[:200])
    if name.startswith("local_"):
        return local_block()["ARP".index(name[-1])]
    raise KeyError(name)


# (name of the matrix, uploaded canonically, packed)
SWEEP_MATRICES = [("33", True, False), ("33", True, True), ("ragged", True, False), ("ragged", True, True),
                  ("local_A", False, False)]


def _mtag(name, canonical, pack):
    return name + ("_packed" if pack else "")


def _vectors(name, *lengths):
    r = rng(sum(map(ord, name)))
    return [r.standard_normal(n) for n in lengths]


# ---- elementwise ops: n = 1, 2, 3 (nothing but the odd tail of the two-per-lane kernels, one pair, a pair and a tail), 1025
# (512 pairs, more than one workgroup of 256 lanes, and a tail) ------------------------------------------------------------------
ELEMENTWISE_N = (1, 2, 3, 1025)


def _axpby(n, kind):
    def inputs():
        r = rng(1, n)
        x, y, alpha, beta = r.standard_normal(n), r.standard_normal(n), 0.7, -1.3
        if kind == "beta0_nan_y":                     # beta == 0: y is stored, not read
            beta, y = 0.0, np.full(n, np.nan)
        if kind == "alpha0_inf_x":                    # alpha == 0 is no special case: 0 * inf is NaN on both sides
            alpha = 0.0
            x[::2] = np.inf
        return dict(x=x, y=y, alpha=alpha, beta=beta)

    def run(s, i):
        s.ops.axpby(i["alpha"], s.ro("x", i["x"]), i["beta"], s.rw("y", i["y"]))
    return Case("%s_n%d" % (kind, n), inputs, run)


def _vmul(n):
    def inputs():
        r = rng(2, n)
        return dict(x=r.standard_normal(n), y=r.standard_normal(n))

    def run(s, i):
        s.ops.vmul(0.8, s.ro("x", i["x"]), s.ro("y", i["y"]), s.rw("out", np.full(n, np.nan)))
    return Case("n%d" % n, inputs, run)


def _vmul_is_the_first_jacobi_sweep():
    """The claim of the kernel's comment: vmul(omega, dinv, b) has the bits of csr_jacobi(A, 0, b, omega)."""
    def inputs():
        A = matrix("33")
        return dict(A=A, b=rng(3).standard_normal(A.shape[0]))

    def run(s, i):
        n = i["A"].shape[0]
        dA = s.csr("A", i["A"])
        dinv = s.ops.csr_inverse_diagonal(dA)
        b = s.ro("b", i["b"])
        s.ops.vmul(0.8, dinv, b, s.rw("by_vmul", np.full(n, np.nan)))
        s.ops.csr_jacobi(dA, s.ro("zero", np.zeros(n)), b, 0.8, s.rw("by_jacobi", np.full(n, np.nan)))
        s.keep("dinv", dinv)

    def post(i, res):
        assert same_bits(res["by_vmul"], res["by_jacobi"]).all() and not np.isnan(res["by_vmul"]).any()
    return Case("first_jacobi_sweep_33", inputs, run, post=post)


def _cheby_update(n, first):
    def inputs():
        r = rng(4, n)
        return dict(dinv=r.standard_normal(n), r=r.standard_normal(n), x=r.standard_normal(n),
                    d=np.full(n, np.nan) if first else r.standard_normal(n))      # first: d is stored, not read

    def run(s, i):
        s.ops.cheby_update(0.3, 1.7, s.ro("dinv", i["dinv"]), s.ro("r", i["r"]), s.rw("d", i["d"]), s.rw("x", i["x"]), first)
    return Case("%s_n%d" % ("first" if first else "later", n), inputs, run)


def _copy(n):
    def run(s, i):
        s.ops.copy(s.ro("src", i["src"]), s.rw("dst", np.full(n, np.nan)))
    return Case("n%d" % n, lambda: dict(src=rng(5, n).standard_normal(n)), run)


def _zero(n):
    def run(s, i):
        s.ops.zero(s.rw("x", i["x"]))
    return Case("n%d" % n, lambda: dict(x=rng(6, n).standard_normal(n)), run)


def _gather(n):
    """buf is five elements longer than idx: they keep what they held."""
    def inputs():
        r = rng(7, n)
        return dict(idx=r.integers(0, n + 7, n).astype(np.int32), x=r.standard_normal(n + 7),
                    buf=np.concatenate([np.full(n, np.nan), r.standard_normal(5)]))

    def run(s, i):
        s.ops.gather(s.ro("idx", i["idx"]), s.ro("x", i["x"]), s.rw("buf", i["buf"]))
    return Case("n%d" % n, inputs, run)


def _scatter(n):
    """buf is five elements longer than idx: they go nowhere.  (The indices are distinct: the order of two stores to one
    element is nobody's contract.)"""
    def inputs():
        r = rng(8, n)
        return dict(idx=r.permutation(n + 7)[:n].astype(np.int32), buf=r.standard_normal(n + 5), x=r.standard_normal(n + 7))

    def run(s, i):
        s.ops.scatter(s.ro("idx", i["idx"]), s.ro("buf", i["buf"]), s.rw("x", i["x"]))
    return Case("n%d" % n, inputs, run)


REGISTRY["axpby"] = Cases([_axpby(n, kind) for n in ELEMENTWISE_N for kind in ("general", "beta0_nan_y", "alpha0_inf_x")])
REGISTRY["vmul"] = Cases([_vmul(n) for n in ELEMENTWISE_N] + [_vmul_is_the_first_jacobi_sweep()])
REGISTRY["cheby_update"] = Cases([_cheby_update(n, first) for n in ELEMENTWISE_N for first in (False, True)])
REGISTRY["copy"] = Cases([_copy(n) for n in ELEMENTWISE_N])
REGISTRY["zero"] = Cases([_zero(n) for n in ELEMENTWISE_N])
REGISTRY["gather"] = Cases([_gather(n) for n in ELEMENTWISE_N])
REGISTRY["scatter"] = Cases([_scatter(n) for n in ELEMENTWISE_N])


# ---- sparse sweeps: the 33 x 33 operator as uploaded and packed, the ragged 321-row matrix (empty rows, rows without a
# diagonal), a non-canonical upload, the rectangular local block of the distributed cycle.  Per-row sums run in storage order
# on both sides: bit for bit.  The vectors are as long as the package passes them: x and b over all layout rows. -------------------
def _spmv(mname, canonical, pack, alpha, beta):
    def inputs():
        A = matrix(mname)
        x, y0 = _vectors(mname, A.shape[1], A.shape[0])
        return dict(A=A, x=x, y=np.full(A.shape[0], np.nan) if beta == 0.0 else y0)

    def run(s, i):
        s.ops.csr_spmv(s.csr("A", i["A"], canonical, pack), s.ro("x", i["x"]), s.rw("y", i["y"]), alpha, beta)
    return Case("%s_a%g_b%g" % (_mtag(mname, canonical, pack), alpha, beta), inputs, run)


def _head_nan(n, m, key):
    """n NaNs (what the op writes) and, for a rectangular block, m - n numbers behind them that must stay."""
    return np.concatenate([np.full(n, np.nan), rng(19, key).standard_normal(m - n)])


def _jacobi(mname, canonical, pack):
    def inputs():
        A = matrix(mname)
        x, b = _vectors(mname, A.shape[1], A.shape[1])
        return dict(A=A, x=x, b=b)

    def run(s, i):
        n, m = i["A"].shape
        s.ops.csr_jacobi(s.csr("A", i["A"], canonical, pack), s.ro("x", i["x"]), s.ro("b", i["b"]), 0.8,
                         s.rw("x_out", _head_nan(n, m, 1)))
    return Case(_mtag(mname, canonical, pack), inputs, run)


def _residual(mname, canonical, pack, with_r):
    """r bit for bit.  norm2 = sum r_i^2: the same n squares (r is the same on both sides) in two orders, so
    |got - stand_in| <= 2 gamma_n sum r_i^2; the bound is evaluated with SciPy's r, inflated by 1e-6 for its own rounding."""
    def inputs():
        A = matrix(mname)
        x, b = _vectors(mname, A.shape[1], A.shape[1])
        return dict(A=A, x=x, b=b)

    def run(s, i):
        n, m = i["A"].shape
        r = s.rw("r", _head_nan(n, m, 2)) if with_r else None
        s.ops.csr_residual_norm2(s.csr("A", i["A"], canonical, pack), s.ro("x", i["x"]), s.ro("b", i["b"]), r,
                                 s.scratch(s.ops.partials_count(n)), s.rw("norm2", np.full(1, np.nan)))

    def bounds(i):
        r = i["b"][:i["A"].shape[0]] - sp.csr_matrix(i["A"]) @ i["x"]
        return dict(norm2=2 * gamma(r.size) * float(r @ r) * (1 + 1e-6))
    return Case("%s_%s" % (_mtag(mname, canonical, pack), "with_r" if with_r else "without_r"), inputs, run, bounds)


def _residual_only_r(mname):
    def inputs():
        A = matrix(mname)
        x, b = _vectors(mname, A.shape[1], A.shape[0])
        return dict(A=A, x=x, b=b)

    def run(s, i):
        s.ops.csr_residual_norm2(s.csr("A", i["A"], False), s.ro("x", i["x"]), s.ro("b", i["b"]),
                                 s.rw("r", np.full(i["A"].shape[0], np.nan)), None, None)
    return Case(mname + "_r_alone", inputs, run)      # (how the distributed cycle calls it)


def _inverse_diagonal(mname, canonical):
    def run(s, i):
        s.keep("dinv", s.ops.csr_inverse_diagonal(s.csr("A", i["A"], canonical)))
    return Case(mname, lambda: dict(A=matrix(mname)), run)


def _gershgorin(mname, canonical):
    """Row sums in storage order on both sides, one division per row, a maximum: bit for bit."""
    def run(s, i):
        s.ops.csr_gershgorin(s.csr("A", i["A"], canonical), s.rw("out", np.full(1, np.nan)))
    return Case(mname, lambda: dict(A=matrix(mname)), run)


REGISTRY["csr_spmv"] = Cases([_spmv(m, c, p, a, b) for m, c, p in SWEEP_MATRICES + [("local_R", False, False), ("local_P", False, False)]
                              for a, b in ALPHA_BETA])
RECTANGULAR = [("ragged_top", True, False)]
REGISTRY["csr_jacobi"] = Cases([_jacobi(m, c, p) for m, c, p in SWEEP_MATRICES + RECTANGULAR])
REGISTRY["csr_residual_norm2"] = Cases([_residual(m, c, p, w) for m, c, p in SWEEP_MATRICES + RECTANGULAR for w in (True, False)]
                                       + [_residual_only_r("local_A")])
DIAGONAL_MATRICES = [("33", True), ("ragged", True), ("33_dupdiag", False), ("local_A", False)]
REGISTRY["csr_inverse_diagonal"] = Cases([_inverse_diagonal(m, c) for m, c in DIAGONAL_MATRICES])
REGISTRY["csr_gershgorin"] = Cases([_gershgorin(m, c) for m, c in DIAGONAL_MATRICES])


# ---- dot, multi_dot, multi_axpy: n = 1, 1089 (odd, several workgroups), SECOND_TRIP; a basis whose row stride exceeds n; k = 0,
# 1, 5 and the most one call takes ------------------------------------------------------------------------------------------------
REDUCTION_N = (1, 1089, SECOND_TRIP)
MAX_K = shim._MAX_VECTORS - 1
KS = (0, 1, 5, MAX_K)


@functools.lru_cache(maxsize=2)
def _basis(n):
    """(V (MAX_K, ldv) with ldv > n and even, w): standard normal, read-only."""
    r = rng(9, n)
    ldv = n + 3 if n % 2 else n + 2
    V, w = r.standard_normal((MAX_K, ldv)), r.standard_normal(n)
    V.setflags(write=False)
    w.setflags(write=False)
    return V, w


def _dot(n):
    """n products in two orders: 2 gamma_n sum |x_i y_i|."""
    def inputs():
        V, w = _basis(n)
        return dict(x=V[0, :n].copy(), y=w)

    def run(s, i):
        s.ops.dot(s.ro("x", i["x"]), s.ro("y", i["y"]), s.scratch(s.ops.partials_count(n)), s.rw("out", np.full(1, np.nan)))
    return Case("n%d" % n, inputs, run, lambda i: dict(out=2 * gamma(n) * float(np.abs(i["x"] * i["y"]).sum())))


def _multi_dot(n, k):
    """out has MAX_K + 1 elements: those from k on stay NaN.  out[j]: 2 gamma_n sum_i |V_ji w_i|."""
    def inputs():
        V, w = _basis(n)
        return dict(V=V, w=w)

    def run(s, i):
        s.ops.multi_dot(s.ro("V", i["V"]), k, s.ro("w", i["w"]), s.scratch(s.ops.multi_partials_count(n, k)),
                        s.rw("out", np.full(MAX_K + 1, np.nan)))

    def bounds(i):
        b = np.zeros(MAX_K + 1)
        b[:k] = 2 * gamma(n) * (np.abs(i["V"][:k, :n]) @ np.abs(i["w"]))
        return dict(out=b)
    return Case("n%d_k%d" % (n, k), inputs, run, bounds)


def _multi_axpy(n, k, subtract, norm, aliased=False):
    """w: every element goes through the same products and sums in the same order on both sides, bit for bit.
    norm2 = sum w_i^2 of that w: 2 gamma_n sum w_i^2.  aliased: coef and norm2 are views of one buffer (how fgmres holds
    h2 and the norm): the coefficients are read before the norm lands."""
    def inputs():
        V, w = _basis(n)
        return dict(V=V, w=w, coef=rng(10, n, k).standard_normal(max(k, 1)))

    def run(s, i):
        V, w = s.ro("V", i["V"]), s.rw("w", i["w"])
        part = s.scratch(s.ops.multi_partials_count(n, k)) if norm else None
        if aliased:
            h = s.rw("h", np.concatenate([i["coef"][:k], [np.nan]]))
            coef, norm2 = h[:k], h[k:k + 1]
        else:
            coef, norm2 = s.ro("coef", i["coef"]), (s.rw("norm2", np.full(1, np.nan)) if norm else None)
        s.ops.multi_axpy(V, k, coef, w, part, norm2, subtract)

    def bounds(i):
        w = i["w"].copy()
        for j in range(k):
            w = w - i["coef"][j] * i["V"][j, :n] if subtract else w + i["coef"][j] * i["V"][j, :n]
        b = 2 * gamma(n) * float(w @ w) * (1 + 1e-6)
        if not norm:
            return {}
        return dict(h=np.concatenate([np.zeros(k), [b]])) if aliased else dict(norm2=b)
    label = "n%d_k%d_%s%s%s" % (n, k, "sub" if subtract else "add", "_norm" if norm else "", "_aliased" if aliased else "")
    return Case(label, inputs, run, bounds)


REGISTRY["dot"] = Cases([_dot(n) for n in REDUCTION_N])
REGISTRY["multi_dot"] = Cases([_multi_dot(n, k) for n in REDUCTION_N for k in KS])
REGISTRY["multi_axpy"] = Cases([_multi_axpy(n, k, sub, norm) for n in REDUCTION_N for k in KS
                                for sub, norm in ((True, True), (False, False))]
                               + [_multi_axpy(1089, 5, True, False), _multi_axpy(1089, 5, False, True),
                                  _multi_axpy(1089, 5, True, True, aliased=True)])


# ---- Gauss-Seidel on a schedule ---------------------------------------------------------------------------------------------------
GS_DEVIATION = ("the stand-ins of csr_gs_schedule and stencil_gs sweep the rows of a schedule in ascending (or descending) order "
                "whatever its sets are, so they are compared on lexicographic schedules only, where that is the exact sweep")


def _gs_schedule(mname, sweeps):
    """The level schedule of the exact forward sweep, built by each side's own build_gs_schedule; with the wavefront kernel
    switched off, as on the levels that run csr_gs_schedule.  Every row update is one sum in storage order: bit for bit."""
    def inputs():
        A = matrix(mname)
        x, b = _vectors(mname + "gs", A.shape[0], A.shape[0])
        return dict(A=A, x=x, b=b)

    def run(s, i):
        from learnmultigrid_amd import ops as real
        dA = s.csr("A", i["A"])
        sched = s.ops.build_gs_schedule(i["A"], "lexicographic", s.device)
        try:
            real.set_wavefront_gs_enabled(False)
            s.ops.csr_gs_schedule(dA, s.rw("x", i["x"]), s.ro("b", i["b"]), sched, sweeps)
        finally:
            real.set_wavefront_gs_enabled(True)
        s.keep("rows_of_the_schedule", np.sort(sched.d_rows.cpu().numpy()))
    return Case("%s_sweeps%d" % (mname, sweeps), inputs, run)


GS_CASES = [_gs_schedule(m, sw) for m in ("33", "33_permuted") for sw in (1, 3)]
REGISTRY["csr_gs_schedule"] = Cases(GS_CASES, deviation=GS_DEVIATION)
REGISTRY["build_gs_schedule"] = Cases(GS_CASES[::2], deviation="the stand-in's schedule holds the rows in ascending order, the "
                                      "product's in the order of its level sets: the same rows, and the same sweep on both sides")


# ---- line relaxation: one x and one y case at the smallest grids of test_line_gpu.py (3 x 5) and test_line_band_gpu.py
# (19 x 13); the arithmetic of line_ref / line_band_ref is the kernels' own, bit for bit ----------------------------------------
def _helix(W, H):
    """x-links that run on across the line ends (test_line_gpu.helix)."""
    return K.as_csr(sp.diags([-1.0, -1.0, 4.5, -1.0, -1.0], [-W, -1, 0, 1, W], shape=(W * H, W * H)).tocsr())


def _line(direction):
    W, H = 3, 5

    def inputs():
        A = LB.window_operator(W, H, 1, seed=31)
        x, r = _vectors("line" + direction, W * H, W * H)
        return dict(A=A, x=x, r=r)

    def run(s, i):
        fac = s.ops.line_factor(s.csr("A", i["A"]), W, direction)
        s.ops.line_solve(W, direction, 1, 2, fac, s.rw("r", i["r"]), 0.8, s.rw("x", i["x"]))
        for name, t in zip(("lo", "minv", "cp"), fac):
            s.keep(name, t)
    return Case("%s_3x5" % direction, inputs, run)


def _line_refusal(what):
    W, H = 3, 5

    def inputs():
        if what == "entry_across_a_line_end":
            return dict(A=_helix(W, H))
        Z = sp.csr_matrix(LB.window_operator(W, H, 1, seed=31)).copy()
        Z.data[:] = np.where(Z.indices == np.repeat(np.arange(W * H), np.diff(Z.indptr)), 0.0, Z.data)   # stored zeros
        return dict(A=Z)

    def run(s, i):
        s.ops.line_factor(s.csr("A", i["A"]), W, "x")
    return Case(what, inputs, run, raises=ValueError)


def _band(direction):
    W, H, p = 19, 13, 2

    def inputs():
        A = LB.window_operator(W, H, p, seed=207)
        x, r = _vectors("band" + direction, W * H, W * H)
        return dict(A=A, x=x, r=r)

    def run(s, i):
        dA = s.csr("A", i["A"])
        fac, flags = s.ops.line_factor_banded_flags(dA, W, direction, p)
        again = s.ops.line_factor_banded(dA, W, direction, p)
        s.ops.line_solve_banded(W, direction, p, 1, 2, again, s.rw("r", i["r"]), 0.8, s.rw("x", i["x"]))
        s.keep("fac", fac)
        s.keep("flags", flags)
        s.keep("fac_again", again)
    return Case("%s_19x13_band2" % direction, inputs, run)


def _band_refusal(what):
    W, H, p = 19, 13, 2

    def inputs():
        A = LB.window_operator(W, H, p, seed=7).tolil()
        if what == "entry_across_a_line_end":
            A[3 * W + 1, 3 * W - 1] = 0.25                    # offset -2 from column 1 of line 3 (test_line_band_gpu.test_flags)
        else:
            i = 5 * W
            A[i, i] = A[i, i + 1] = A[i + 1, i] = A[i + 1, i + 1] = 1.0        # a singular leading block of x-line 5
        return dict(A=K.as_csr(sp.csr_matrix(A)))

    def run(s, i):
        s.ops.line_factor_banded(s.csr("A", i["A"]), W, "x", p)
    return Case(what, inputs, run, raises=ValueError)


LINE_CASES = [_line("x"), _line("y")]
REGISTRY["line_factor"] = Cases(LINE_CASES + [_line_refusal("entry_across_a_line_end"), _line_refusal("zero_pivot")])
REGISTRY["line_solve"] = Cases(LINE_CASES)
BAND_CASES = [_band("x"), _band("y")]
REGISTRY["line_factor_banded_flags"] = Cases(BAND_CASES)
REGISTRY["line_factor_banded"] = Cases(BAND_CASES + [_band_refusal("entry_across_a_line_end"), _band_refusal("zero_pivot")])
REGISTRY["line_solve_banded"] = Cases(BAND_CASES)


# ---- SpGEMM ------------------------------------------------------------------------------------------------------------------------
def _spgemm(which):
    """R @ A and (R A) @ P on the 33 x 33 operator and its tensor transfer; the second product takes the SAME left factor on
    both sides (SciPy's R A, sorted).  The patterns -- sorted rows -- are equal exactly.  An entry of C is a sum of at most m
    products, m the longest row of the left factor, taken in SciPy's order or the kernel's: 2 gamma_m (|A| |B|)_ij.
    numeric(A, B, out=C) returns C itself: its values are NaN before the call."""
    def inputs():
        A, Pm, R = operators(33, "5pt")
        if which == "RA":
            return dict(A=R, B=A)
        RA = sp.csr_matrix(R @ A)
        RA.sort_indices()
        return dict(A=K.as_csr(RA), B=Pm)

    def run(s, i):
        dA, dB = s.csr("A", i["A"]), s.csr("B", i["B"])
        plan = s.ops.SpGEMMPlan(dA, dB)
        C = plan.numeric(dA, dB)
        assert tuple(C.shape) == (i["A"].shape[0], i["B"].shape[1]) == tuple(plan.shape)
        for name, t in (("rowptr", C.rowptr), ("colidx", C.colidx), ("vals", C.vals)):
            s.keep(name, t.clone())
        C.vals.fill_(float("nan"))
        again = plan.numeric(dA, dB, out=C)
        assert again is C
        for name, t in (("rowptr_out", C.rowptr), ("colidx_out", C.colidx), ("vals_out", C.vals)):
            s.keep(name, t.clone())

    def bounds(i):
        T = sp.csr_matrix(abs(sp.csr_matrix(i["A"])) @ abs(sp.csr_matrix(i["B"])))
        T.sort_indices()
        b = 2 * gamma(int(np.diff(sp.csr_matrix(i["A"]).indptr).max())) * T.data
        return dict(vals=b, vals_out=b)
    return Case(which, inputs, run, bounds)


REGISTRY["SpGEMMPlan"] = Cases([_spgemm("RA"), _spgemm("RAP")], deviation="the stand-in ignores `record`: it multiplies afresh "
                               "in every call, the plan of the product replays a recorded map from its second call on")


# ---- the fused passes: the existing tests hold them to the oracle bit for bit, and so does this --------------------------------
FUSED_OPERATORS = ((65, "5pt"), (33, "9pt"))
REFUSAL = "the real predicate %s refuses the %d x %d %s operator (ops.TILED_MIN_ROWS and the register-pass thresholds)"


@functools.lru_cache(maxsize=None)
def _fused_inputs(side, kind):
    A, Pm, R = operators(side, kind)
    r = rng(11, side)
    return dict(A=A, P=Pm, R=R, x=r.standard_normal(A.shape[0]), b=r.standard_normal(A.shape[0]),
                e=r.standard_normal(Pm.shape[1]))


def _fused(op, form, side, kind, arg):
    """form: plain | zero (x_in None) | prolong | restrict | turnaround | cheby (arg: the degree) | gs (arg: the direction)."""
    def run(s, i):
        from learnmultigrid_amd import ops as real
        n, nc = i["A"].shape[0], i["P"].shape[1]
        dA = s.csr("A", i["A"], pack=True)
        b = s.ro("b", i["b"])
        refused = lambda name: REFUSAL % (name, side, side, kind)
        if form == "gs":
            s.require(real.stencil_gs_available(dA, arg), refused("stencil_gs_available"))
            s.ops.stencil_gs(dA, s.rw("x", i["x"]), b, 2, arg)
            if s.on_device:
                real.stencil_gs_check(dA)
            return
        if form == "cheby":
            s.require(real.stencil_cheby_available(dA), refused("stencil_cheby_available"))
            s.ops.stencil_cheby(dA, s.ro("x", i["x"]), b, CR.coefficients(2.0, 4.0, arg), s.rw("x_out", np.full(n, np.nan)),
                                s.rw("r_out", np.full(n, np.nan)))
            return
        s.require(real.stencil_smooth_available(dA), refused("stencil_smooth_available"))
        x_out = s.rw("x_out", np.full(n, np.nan))
        if form == "plain":
            s.ops.stencil_smooth(dA, s.ro("x", i["x"]), b, 0.8, 2, x_out, s.rw("r_out", np.full(n, np.nan)))
        elif form == "zero":
            s.ops.stencil_smooth(dA, None, b, 0.8, 3, x_out)
        else:
            dP, dR = s.csr("P", i["P"], pack=True), s.csr("R", i["R"], pack=True)
            e, bc = s.ro("e", i["e"]), s.rw("b_coarse", np.full(nc, np.nan))
            if form == "prolong":
                s.require(real.stencil_smooth_prolong_available(dA, dP), refused("stencil_smooth_prolong_available"))
                s.ops.stencil_smooth(dA, s.ro("x", i["x"]), b, 0.8, 2, x_out, prolong=(dP, e))
            elif form == "restrict":
                s.require(real.stencil_smooth_restrict_available(dA, dR), refused("stencil_smooth_restrict_available"))
                s.ops.stencil_smooth(dA, s.ro("x", i["x"]), b, 0.8, 2, x_out, restrict=(dR, bc))
            else:
                # (stencil_smooth_turnaround_selected adds a size window measured for speed to this; the pass itself runs
                # wherever stencil_smooth_turnaround_available says so)
                s.require(real.stencil_smooth_turnaround_available(dA, dP, dR), refused("stencil_smooth_turnaround_available"))
                s.ops.stencil_smooth_turnaround(dA, s.ro("x", i["x"]), b, 0.8, 2, 1, x_out, (dP, e), (dR, bc))
    label = "%s%s_%d_%s" % (form, "" if arg is None else "_%s" % arg, side, kind)
    return Case(label, lambda: _fused_inputs(side, kind), run)


FUSED_CASES = {
    "stencil_smooth": [_fused("stencil_smooth", f, s, k, None) for s, k in FUSED_OPERATORS for f in ("plain", "zero", "prolong", "restrict")],
    "stencil_smooth_turnaround": [_fused("stencil_smooth_turnaround", "turnaround", s, k, None) for s, k in FUSED_OPERATORS],
    "stencil_cheby": [_fused("stencil_cheby", "cheby", s, k, d) for s, k in FUSED_OPERATORS for d in (1, 2, 3)],
    "stencil_gs": [_fused("stencil_gs", "gs", s, k, d) for s, k in FUSED_OPERATORS for d in ("forward", "backward")],
}
REGISTRY["stencil_smooth"] = Cases(FUSED_CASES["stencil_smooth"])
# (fused("cheby") offers a turnaround that raises on purpose: the Chebyshev cycle must not pick it up)
REGISTRY["stencil_smooth_turnaround"] = Cases(FUSED_CASES["stencil_smooth_turnaround"], only=("fused_jacobi", "fused_all"))
REGISTRY["stencil_cheby"] = Cases(FUSED_CASES["stencil_cheby"])
REGISTRY["stencil_gs"] = Cases(FUSED_CASES["stencil_gs"], deviation=GS_DEVIATION)


# ---- block ops, k = 2, 4, 8 -----------------------------------------------------------------------------------------------------
BLOCK_N = 1089                  # odd, several workgroups of the fixed 1024 x 256 geometry's map


def _block_inputs(k, seed):
    A = matrix("ragged")
    r = rng(12, k, seed)
    return dict(A=A, X=r.standard_normal((A.shape[1], k)), B=r.standard_normal((A.shape[0], k)),
                Y=r.standard_normal((A.shape[0], k)))


def _block_terms(i, k):
    """|B| + |A| |X| entry by entry, and the longest row m: each side's B - A X carries at most gamma_(m+1) of it."""
    A = sp.csr_matrix(i["A"])
    return np.abs(i["B"]) + abs(A) @ np.abs(i["X"]), int(np.diff(A.indptr).max())


def _block_residual(k, with_r):
    """R = B - A X: a sum of m + 1 terms per entry, SciPy's order against the sliced-ELL kernel's: E = 2 gamma_(m+1)
    (|B| + |A| |X|).  norm2[j] = sum_i R_ij^2 of each side's own R: |sum (R + d)^2 - sum R^2| <= sum (2 |R| |d| + d^2) with
    |d| <= E, plus 2 gamma_n sum (|R| + E)^2 for the order of the n squares.  norm2 has k + 2 elements: two stay NaN."""
    def run(s, i):
        n = i["A"].shape[0]
        S = s.ops.block_twin(s.csr("A", i["A"]))
        R = s.rw("R", np.full((n, k), np.nan)) if with_r else None
        s.ops.block_residual_norm2(S, s.ro("X", i["X"]), s.ro("B", i["B"]), R, s.scratch(s.ops.block_partials_count(n, k)),
                                   s.rw("norm2", np.full(k + 2, np.nan)))

    def bounds(i):
        t, m = _block_terms(i, k)
        E = 2 * gamma(m + 1) * t
        R = np.abs(i["B"] - sp.csr_matrix(i["A"]) @ i["X"]) + E
        n2 = (2 * R * E + E * E).sum(axis=0) + 2 * gamma(R.shape[0]) * (R * R).sum(axis=0)
        out = dict(norm2=np.concatenate([n2, [0.0, 0.0]]))
        if with_r:
            out["R"] = E
        return out
    return Case("k%d_%s" % (k, "with_R" if with_r else "without_R"), lambda: _block_inputs(k, 0), run, bounds)


def _block_jacobi(k):
    """Out = X + omega ((1 / d) (B - A X)): the residual's m + 1 terms and five more roundings (the reciprocal, two products,
    the sum, and one to spare for another association of omega / d), each of which either side may take in its own order:
    2 gamma_(m+6) (|X| + |omega / d| (|B| + |A| |X|)).  A row without a diagonal keeps X on both sides: bit for bit."""
    def run(s, i):
        S = s.ops.block_twin(s.csr("A", i["A"]))
        s.ops.block_jacobi(S, s.ro("X", i["X"]), s.ro("B", i["B"]), 0.8, s.rw("Out", np.full(i["B"].shape, np.nan)))

    def bounds(i):
        t, m = _block_terms(i, k)
        d = sp.csr_matrix(i["A"]).diagonal()[:, None]
        with np.errstate(divide="ignore"):
            return dict(Out=np.where(d != 0, 2 * gamma(m + 6) * (np.abs(i["X"]) + np.abs(0.8 / d) * t), 0.0))
    return Case("k%d" % k, lambda: _block_inputs(k, 1), run, bounds)


def _block_spmv(k, alpha, beta):
    """Y = alpha A X + beta Y: m products, the two scalings and the sum: 2 gamma_(m+3) (|alpha| |A| |X| + |beta| |Y|).
    beta == 0: Y is stored, not read (it holds NaN)."""
    def inputs():
        i = dict(_block_inputs(k, 2))
        if beta == 0.0:
            i["Y"] = np.full(i["Y"].shape, np.nan)
        return i

    def run(s, i):
        S = s.ops.block_twin(s.csr("A", i["A"]))
        s.ops.block_spmv(S, s.ro("X", i["X"]), s.rw("Y", i["Y"]), alpha, beta)

    def bounds(i):
        A = sp.csr_matrix(i["A"])
        t = abs(alpha) * (abs(A) @ np.abs(i["X"])) + (abs(beta) * np.abs(i["Y"]) if beta != 0.0 else 0.0)
        return dict(Y=2 * gamma(int(np.diff(A.indptr).max()) + 3) * t)
    return Case("k%d_a%g_b%g" % (k, alpha, beta), inputs, run, bounds)


def _dense_gemv_block(k):
    """Y = M X, M 37 x 23 (odd both ways: the element path of the row kernel, rows that fill no wave evenly): an entry is 23
    products in BLAS's order or the wave's: 2 gamma_23 (|M| |X|)."""
    def inputs():
        r = rng(13, k)
        return dict(M=r.standard_normal((37, 23)), X=r.standard_normal((23, k)))

    def run(s, i):
        s.ops.dense_gemv_block(s.ro("M", i["M"]), s.ro("X", i["X"]), s.rw("Y", np.full((37, k), np.nan)))
    return Case("k%d_37x23" % k, inputs, run, lambda i: dict(Y=2 * gamma(23) * (np.abs(i["M"]) @ np.abs(i["X"]))))


def _block_dot(k, n):
    """out[j]: n products in two orders, 2 gamma_n sum_i |X_ij Y_ij|; out has k + 2 elements, two stay NaN."""
    def inputs():
        r = rng(14, k, n)
        return dict(X=r.standard_normal((n, k)), Y=r.standard_normal((n, k)))

    def run(s, i):
        s.ops.block_dot(s.ro("X", i["X"]), s.ro("Y", i["Y"]), s.scratch(s.ops.block_dot_partials_count(n, k)),
                        s.rw("out", np.full(k + 2, np.nan)))

    def bounds(i):
        return dict(out=np.concatenate([2 * gamma(n) * np.abs(i["X"] * i["Y"]).sum(axis=0), [0.0, 0.0]]))
    return Case("k%d_n%d" % (k, n), inputs, run, bounds)


def _block_cg_step(k, edge):
    """X and R: axpby's products and sums on both sides, bit for bit; a column that is off holds NaN everywhere and comes
    back as it went.  rr[j] = sum R_ij^2 of that R: 2 gamma_n sum R_ij^2 (NaN for the NaN column on both sides).  The masks
    are equal exactly: the thresholds are 0 (stays on) and 1e300 (goes off), far from every rr.
    edge "off": column 1 is off and holds NaN in P and AP, numbers in X and R that must come back as they went (a side that
    ignores the mask turns them into NaN); for k > 2 column 2 is off and holds NaN in all four blocks.
    edge "pAp0": column 0 has pAp == 0, so alpha = 0 and nothing is divided."""
    n = BLOCK_N

    def inputs():
        r = rng(15, k)
        i = {name: r.standard_normal((n, k)) for name in ("P", "AP", "X", "R")}
        i.update(rz=r.uniform(0.5, 2.0, k), pAp=r.uniform(0.5, 2.0, k), tol2=np.zeros(k), mask=np.ones(k))
        i["tol2"][-1] = 1e300
        if edge == "off":
            i["mask"][1] = 0.0
            i["P"][:, 1] = i["AP"][:, 1] = np.nan             # read although the column is off: X and R turn NaN
            if k > 2:
                i["mask"][2] = 0.0
                for name in ("P", "AP", "X", "R"):
                    i[name][:, 2] = np.nan
        else:
            i["pAp"][0] = 0.0
        return i

    def run(s, i):
        s.ops.block_cg_step(s.ro("rz", i["rz"]), s.ro("pAp", i["pAp"]), s.ro("tol2", i["tol2"]), s.rw("mask", i["mask"]),
                            s.ro("P", i["P"]), s.ro("AP", i["AP"]), s.rw("X", i["X"]), s.rw("R", i["R"]),
                            s.scratch(s.ops.block_dot_partials_count(n, k)), s.rw("rr", np.full(k, np.nan)))

    def bounds(i):
        on = i["mask"] != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = np.where(on & (i["pAp"] != 0), i["rz"] / i["pAp"], 0.0)
        R = np.where(on[None, :], -alpha[None, :] * i["AP"] + i["R"], i["R"])
        return dict(rr=np.nan_to_num(2 * gamma(n) * (R * R).sum(axis=0) * (1 + 1e-6)))
    return Case("k%d_%s" % (k, edge), inputs, run, bounds)


def _block_cg_direction(k, edge):
    """P = Z + beta P, axpby's bits on both sides.  edge "beta0": rz_new[0] == 0 over a P column of NaN -- beta == 0 stores Z
    and does not read P (csrc/krylov.hip).  edge "off": column 1 is off and holds NaN in Z, numbers in P that must come back as
    they went; for k > 2 column 2 is off and holds NaN in both."""
    n = BLOCK_N

    def inputs():
        r = rng(16, k)
        i = dict(Z=r.standard_normal((n, k)), P=r.standard_normal((n, k)), rz_new=r.uniform(0.5, 2.0, k),
                 rz_old=r.uniform(0.5, 2.0, k), mask=np.ones(k))
        if edge == "beta0":
            i["rz_new"][0] = 0.0
            i["P"][:, 0] = np.nan
        else:
            i["mask"][1] = 0.0
            i["Z"][:, 1] = np.nan
            if k > 2:
                i["mask"][2] = 0.0
                i["Z"][:, 2] = i["P"][:, 2] = np.nan
        return i

    def run(s, i):
        s.ops.block_cg_direction(s.ro("rz_new", i["rz_new"]), s.ro("rz_old", i["rz_old"]), s.ro("mask", i["mask"]),
                                 s.ro("Z", i["Z"]), s.rw("P", i["P"]))

    def post(i, res):
        if edge == "beta0":
            assert same_bits(res["P"][:, 0], i["Z"][:, 0]).all()
    return Case("k%d_%s" % (k, edge), inputs, run, post=post)


BASIS_BLOCKS = 4


def _block_basis(k):
    r = rng(17, k)
    return dict(V=r.standard_normal((BASIS_BLOCKS, BLOCK_N, k)), W=r.standard_normal((BLOCK_N, k)),
                coef=r.standard_normal(BASIS_BLOCKS * k))


def _block_multi_dot(k, nb):
    """out[i k + j]: n products in two orders, 2 gamma_n sum |V_i[:, j] W[:, j]|; what lies behind nb k stays NaN."""
    def run(s, i):
        s.ops.block_multi_dot(s.ro("V", i["V"]), nb, s.ro("W", i["W"]),
                              s.scratch(s.ops.block_multi_partials_count(BLOCK_N, k, nb)),
                              s.rw("out", np.full(BASIS_BLOCKS * k + 2, np.nan)))

    def bounds(i):
        b = np.zeros(BASIS_BLOCKS * k + 2)
        b[:nb * k] = (2 * gamma(BLOCK_N) * np.abs(i["V"][:nb] * i["W"][None]).sum(axis=1)).reshape(-1)
        return dict(out=b)
    return Case("k%d_nb%d" % (k, nb), lambda: _block_basis(k), run, bounds)


def _block_multi_axpy(k, subtract, norm):
    """W bit for bit (multi_axpy's loop column by column); the column with a count of 0 holds NaN and is not stored.
    norm2[j] = sum W_ij^2 of that W: 2 gamma_n sum W_ij^2, NaN for the NaN column on both sides."""
    counts = [0 if j == 1 else min(BASIS_BLOCKS, 1 + j) for j in range(k)]

    def inputs():
        i = dict(_block_basis(k))
        i["W"] = i["W"].copy()
        i["W"][:, 1] = np.nan
        return i

    def run(s, i):
        part = s.scratch(s.ops.block_multi_partials_count(BLOCK_N, k, 1)) if norm else None
        s.ops.block_multi_axpy(s.ro("V", i["V"]), counts, s.ro("coef", i["coef"]), s.rw("W", i["W"]), part,
                               s.rw("norm2", np.full(k + 2, np.nan)) if norm else None, subtract)

    def bounds(i):
        if not norm:
            return {}
        W = i["W"].copy()
        for j in range(k):
            for b in range(counts[j]):
                W[:, j] = W[:, j] + (-1.0 if subtract else 1.0) * i["coef"][b * k + j] * i["V"][b, :, j]
        return dict(norm2=np.concatenate([np.nan_to_num(2 * gamma(BLOCK_N) * (W * W).sum(axis=0) * (1 + 1e-6)), [0.0, 0.0]]))
    return Case("k%d_%s%s" % (k, "sub" if subtract else "add", "_norm" if norm else ""), inputs, run, bounds)


def _block_scale(k):
    """One product per element; a scale of 0 stores +0.0 over a column of NaN."""
    scale = [0.0 if j == 1 else (-1.0) ** j * (0.5 + j) for j in range(k)]

    def inputs():
        W = _block_basis(k)["W"].copy()
        W[:, 1] = np.nan
        return dict(W=W)

    def run(s, i):
        s.ops.block_scale(scale, s.rw("W", i["W"]))

    def post(i, res):
        assert same_bits(res["W"][:, 1], np.zeros(BLOCK_N)).all()
    return Case("k%d" % k, inputs, run, post=post)


REGISTRY["block_residual_norm2"] = Cases([_block_residual(k, w) for k in WIDTHS for w in (True, False)])
REGISTRY["block_jacobi"] = Cases([_block_jacobi(k) for k in WIDTHS])
REGISTRY["block_spmv"] = Cases([_block_spmv(k, a, b) for k in WIDTHS for a, b in ((1.0, 0.0), (-0.5, 2.0))])
REGISTRY["dense_gemv_block"] = Cases([_dense_gemv_block(k) for k in WIDTHS])
REGISTRY["block_dot"] = Cases([_block_dot(k, n) for k in WIDTHS for n in REDUCTION_N])
REGISTRY["block_cg_step"] = Cases([_block_cg_step(k, e) for k in WIDTHS for e in ("off", "pAp0")])
REGISTRY["block_cg_direction"] = Cases([_block_cg_direction(k, e) for k in WIDTHS for e in ("beta0", "off")])
REGISTRY["block_multi_dot"] = Cases([_block_multi_dot(k, nb) for k in WIDTHS for nb in (0, 3)])
REGISTRY["block_multi_axpy"] = Cases([_block_multi_axpy(k, sub, norm) for k in WIDTHS for sub, norm in ((True, True), (False, False))])
REGISTRY["block_scale"] = Cases([_block_scale(k) for k in WIDTHS])


# ---- covered elsewhere, or nothing to compare ---------------------------------------------------------------------------------
for _op, _test in (("dense_gemv_blockdiag", "test_shim_dense_gemv_blockdiag"), ("dense_gemv_windows", "test_shim_dense_gemv_windows"),
                   ("dense_gemv_windows_off", "test_shim_dense_gemv_windows_off"),
                   ("coarse_front_gather", "test_shim_coarse_front_gather"), ("coarse_back_gather", "test_shim_coarse_back_gather"),
                   ("block_copy", "test_shim_block_copy")):
    REGISTRY[_op] = CoveredBy("test_coarse_kernels_gpu.py::" + _test)

REGISTRY["DeviceCSR"] = NoValues("the package's own container, re-exported: it holds CPU tensors as it holds device tensors")
REGISTRY["partials_count"] = NoValues("size helper: how much scratch a reduction of the stand-in would take; the scratch is never read")
REGISTRY["multi_partials_count"] = NoValues("size helper of multi_dot / multi_axpy's scratch")
REGISTRY["block_partials_count"] = NoValues("size helper of the block sweeps' scratch")
REGISTRY["block_dot_partials_count"] = NoValues("size helper of block_dot / block_cg_step's scratch")
REGISTRY["block_multi_partials_count"] = NoValues("size helper of the block Gram-Schmidt ops' scratch")
REGISTRY["krylov_max_vectors"] = NoValues("a constant, checked on the CPU: test_shim_signatures_cpu.test_constants_equal_the_library")
REGISTRY["block_twin"] = NoValues("on the CPU a twin is the matrix itself; every block sweep case goes through it on both sides")
for _op in ("stencil_smooth_available", "stencil_smooth_prolong_available", "stencil_smooth_restrict_available",
            "stencil_smooth_turnaround_selected", "stencil_cheby_available", "stencil_cheby_prolong_available",
            "stencil_cheby_restrict_available", "stencil_gs_available"):
    REGISTRY[_op] = NoValues("a test knob of the fused namespaces (max_rows, turnaround): says which levels a trace runs fused")
REGISTRY["stencil_gs_check"] = NoValues("the stand-in has no wavefront bands that could time out: it returns None")
# dense_gemv has no test_shim_* test: the smallest dense blocks of the coarse solve, against the oracle's own row product


def _dense_gemv(rows, cols):
    """The stand-in is the oracle's row product, which the kernel's wave sums in another order: 2 gamma_cols (|M| |x|)."""
    def inputs():
        r = rng(18, rows, cols)
        return dict(M=r.standard_normal((rows, cols)), x=r.standard_normal(cols))

    def run(s, i):
        s.ops.dense_gemv(s.ro("M", i["M"]), s.ro("x", i["x"]), s.rw("y", np.full(rows, np.nan)))
    return Case("%dx%d" % (rows, cols), inputs, run, lambda i: dict(y=2 * gamma(cols) * (np.abs(i["M"]) @ np.abs(i["x"]))))


# (from 1024 columns on a matrix of up to 8192 rows runs the workgroup-per-row kernel)
REGISTRY["dense_gemv"] = Cases([_dense_gemv(1, 1), _dense_gemv(37, 23), _dense_gemv(81, 81), _dense_gemv(33, 1024)])


def parameters():
    """[(op, case)] of every case of the registry, in registry order."""
    return [(op, c) for op, e in REGISTRY.items() if isinstance(e, Cases) for c in e.cases]
