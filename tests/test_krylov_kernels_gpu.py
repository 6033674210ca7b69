"""The fused Gram-Schmidt kernels (csrc/krylov.hip) against NumPy (-m gpu): lmg_multi_dot within the bar of lmg_dot and bit
for bit independent of k and of the other columns, lmg_multi_axpy bit for bit against the NumPy loop with its coefficients
read from the device, the padding of the bases never touched, the argument checks, and the two torch ops.

Shapes: n = 1, 2 (no pair / one pair), 255, 257 (around one workgroup), 4099 (odd, several workgroups), 262147 and
1000003 (one and several steps of the 1024 x 256 grid-stride, odd); k around the 16 columns one lane keeps in flight
(1, 2, 7, 8, 9, 33) and the most a call takes; ldv = n rounded up to even, and that plus 6 (n + 6 itself is odd for an odd n,
which the C ABI refuses: a row stride must keep every row on 16 bytes)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from learnmultigrid_amd import _lib, ops   # noqa: E402
from support import DEV                    # noqa: E402

F64 = torch.float64
NS = (1, 2, 255, 257, 4099, 262147, 1000003)
MAXK = "max"
KS = (1, 2, 7, 8, 9, 33, MAXK)


def bits(t):
    return t.view(torch.int64)


def spread(rng, size):
    """Entries over 1e-8 .. 1e+8 with random signs: a summation-order mistake moves the result far beyond the bar."""
    return rng.choice((-1.0, 1.0), size) * 10.0 ** rng.uniform(-8.0, 8.0, size)


class Case:
    """A basis of k rows (one NaN row after them, NaN padding from n to ldv) and a vector w inside a NaN-padded allocation."""

    def __init__(self, n, k, pad):
        self.n, self.k = n, k
        self.ldv = n + (n & 1) + (0 if pad == "even" else 6)
        rng = np.random.default_rng(1000 * k + n % 997)
        step = 977
        pool = spread(rng, n + step * k)                          # row j = a window of the pool: cheap, all rows differ
        self.V = np.full((k + 1, self.ldv), np.nan)
        for j in range(k):
            self.V[j, :n] = pool[step * j:step * j + n]
        self.w = spread(rng, n)
        self.dV = torch.from_numpy(self.V).to(DEV)
        self.V_bits = bits(self.dV).clone()

    def dw(self):
        """A fresh device copy of w at the start of an ldv-long allocation whose rest is NaN."""
        full = torch.full((self.ldv,), float("nan"), dtype=F64, device=DEV)
        full[:self.n] = torch.from_numpy(self.w).to(DEV)
        return full, full[:self.n]

    def scratch(self, k=None):
        k = self.k if k is None else k
        return (torch.full((ops.multi_partials_count(self.n, k),), 123.0, dtype=F64, device=DEV),
                torch.full((max(k, 1),), float("nan"), dtype=F64, device=DEV))

    def untouched(self, w_full=None):
        assert torch.equal(bits(self.dV), self.V_bits)
        if w_full is not None:
            assert bool(torch.isnan(w_full[self.n:]).all())


@pytest.fixture(scope="module", params=[(n, k, pad) for n in NS for k in KS for pad in ("even", "plus6")],
                ids=lambda p: "n%d-k%s-%s" % p)
def case(request):
    n, k, pad = request.param
    return Case(n, ops.krylov_max_vectors() if k == MAXK else k, pad)


def test_max_vectors_allows_restart_64():
    assert ops.krylov_max_vectors() >= 65
    assert ops.multi_partials_count(1000, 3) >= 3


# ---- 7. multi_dot ----------------------------------------------------------------------------------------------------------
def test_multi_dot(case):
    n, k = case.n, case.k
    w_full, w = case.dw()
    part, out = case.scratch()
    ops.multi_dot(case.dV, k, w, part, out)
    got = out.cpu().numpy()
    want = case.V[:k, :n] @ case.w
    bar = 1e-13 * (np.abs(case.V[:k, :n]) @ np.abs(case.w))
    print("n %d k %d: max |got - want| / (|V_j| . |w|) = %.3e" % (n, k, (np.abs(got - want) / (bar / 1e-13)).max()))
    assert np.isfinite(got).all() and (np.abs(got - want) <= bar).all()
    # column j alone, as a k = 1 call on its row: the same bits
    part1, out1 = case.scratch(1)
    for j in range(k):
        ops.multi_dot(case.dV[j:j + 1], 1, w, part1, out1)
        assert torch.equal(bits(out1), bits(out[j:j + 1])), j
    # the other rows permuted: every column keeps its bits
    perm = np.random.default_rng(k).permutation(k)
    dVp = case.dV.clone()
    dVp[:k] = case.dV[torch.from_numpy(perm).to(DEV)]
    part2, outp = case.scratch()
    ops.multi_dot(dVp, k, w, part2, outp)
    assert torch.equal(bits(outp), bits(out[torch.from_numpy(perm).to(DEV)]))
    case.untouched(w_full)
    assert np.array_equal(w.cpu().numpy(), case.w)


# ---- 8. multi_axpy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subtract", [True, False])
def test_multi_axpy(case, subtract):
    n, k = case.n, case.k
    w_full, w = case.dw()
    part, h = case.scratch()
    norm2 = torch.full((1,), float("nan"), dtype=F64, device=DEV)
    ops.multi_dot(case.dV, k, w, part, h)                      # the coefficients stay on the device ...
    ops.multi_axpy(case.dV, k, h, w, part, norm2, subtract=subtract)     # ... and are read from there, same stream
    c = h.cpu().numpy()
    want = case.w.copy()
    for j in range(k):
        want = want - c[j] * case.V[j, :n] if subtract else want + c[j] * case.V[j, :n]
    got = w.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(got, want)
    n2 = float(want @ want)
    print("n %d k %d subtract %s: |norm2 - want| / want = %.3e" % (n, k, subtract, abs(norm2.item() - n2) / n2))
    assert abs(norm2.item() - n2) <= 1e-13 * n2
    case.untouched(w_full)
    # without the norm the scratch is not written
    w_full, w = case.dw()
    part2 = torch.full_like(part, 123.0)
    ops.multi_axpy(case.dV, k, h, w, part2, None, subtract=subtract)
    assert np.array_equal(w.cpu().numpy(), want)
    assert bool((part2 == 123.0).all())
    w_full, w = case.dw()
    ops.multi_axpy(case.dV, k, h, w, subtract=subtract)
    assert np.array_equal(w.cpu().numpy(), want)
    case.untouched(w_full)


def test_norm_of_an_unchanged_vector():
    """k = 0 with a norm: w keeps its bits and |w|^2 comes out."""
    rng = np.random.default_rng(3)
    x = spread(rng, 4099)
    w = torch.from_numpy(x).to(DEV)
    V = torch.full((1, 4100), float("nan"), dtype=F64, device=DEV)
    part = torch.empty(ops.multi_partials_count(4099, 0), dtype=F64, device=DEV)
    n2 = torch.zeros(1, dtype=F64, device=DEV)
    ops.multi_axpy(V, 0, torch.zeros(1, dtype=F64, device=DEV), w, part, n2)
    assert np.array_equal(w.cpu().numpy(), x)
    assert abs(n2.item() - float(x @ x)) <= 1e-13 * float(x @ x)


# ---- 9. argument checks ----------------------------------------------------------------------------------------------------
def test_argument_checks():
    L = _lib.lib()
    kmax = L.lmg_krylov_max_vectors()
    n, k, ldv = 100, 3, 100
    V = torch.ones((k, ldv + 2), dtype=F64, device=DEV)
    w = torch.ones(n + 2, dtype=F64, device=DEV)
    part = torch.zeros(L.lmg_multi_partials_count(n, kmax), dtype=F64, device=DEV)
    out = torch.full((kmax,), float("nan"), dtype=F64, device=DEV)
    pV, pw, pp, po = V.data_ptr(), w.data_ptr(), part.data_ptr(), out.data_ptr()
    ARG, ALIGN = -1, -2

    def dot(n=n, k=k, V=pV, ldv=ldv, w=pw, part=pp, out=po):
        return L.lmg_multi_dot(n, k, V, ldv, w, part, out, None)

    def axpy(n=n, k=k, V=pV, ldv=ldv, coef=po, w=pw, part=pp, norm2=po + 8 * (kmax - 1)):
        return L.lmg_multi_axpy(n, k, 1, V, ldv, coef, w, part, norm2, None)

    for call in (dot, axpy):
        assert call(V=None) == ARG and call(w=None) == ARG
        assert call(k=-1) == ARG and call(k=kmax + 1) == ARG and call(n=-1) == ARG
        assert call(ldv=101) == ARG                 # odd
        assert call(ldv=98) == ARG                  # < n
        assert call(V=pV + 8) == ALIGN and call(w=pw + 8) == ALIGN
    assert dot(out=None) == ARG and dot(part=None) == ARG
    assert axpy(coef=None) == ARG and axpy(part=None) == ARG
    # nothing to do
    assert dot(k=0, V=None, out=None, part=None) == 0
    assert dot(n=0, V=None, w=None) == 0
    torch.cuda.synchronize()
    assert not out[:k].cpu().numpy().any() and bool(torch.isnan(out[k:]).all())
    n2 = torch.full((1,), float("nan"), dtype=F64, device=DEV)
    assert axpy(n=0, V=None, w=None, norm2=n2.data_ptr()) == 0
    assert n2.item() == 0.0
    assert axpy(n=0, V=None, w=None, part=None, norm2=None) == 0
    assert axpy(k=0, V=None, coef=None, part=None, norm2=None) == 0
    assert bool((V == 1.0).all()) and bool((w == 1.0).all())
    # the wrappers refuse what the C ABI cannot see
    with pytest.raises(ValueError):
        ops.multi_dot(V, k + 1, w[:n], part, out)
    with pytest.raises(ValueError):
        ops.multi_dot(V, k, w[:n], part, out[:k - 1])
    with pytest.raises(TypeError):
        ops.multi_dot(V[:, :ldv], k, w[:n], part, out)          # not contiguous
    with pytest.raises(_lib.LmgError):
        ops.multi_dot(torch.ones((k, ldv + 1), dtype=F64, device=DEV), k, w[:n], part, out)      # odd row stride


# ---- 10. torch ops ---------------------------------------------------------------------------------------------------------
def test_torch_ops_return_what_the_wrappers_do():
    ops.register_torch_ops()
    c = Case(4099, 9, "plus6")
    _, w = c.dw()
    part, out = c.scratch()
    ops.multi_dot(c.dV, 9, w, part, out)
    h = torch.ops.lmg.multi_dot(c.dV, 9, w)
    assert h.shape == (9,) and torch.equal(bits(h), bits(out))
    for subtract in (True, False):
        _, w1 = c.dw()
        _, w2 = c.dw()
        n2 = torch.zeros(1, dtype=F64, device=DEV)
        ops.multi_axpy(c.dV, 9, out, w1, part, n2, subtract=subtract)
        got = torch.ops.lmg.multi_axpy_(c.dV, 9, h, w2, subtract)
        assert got.shape == (1,) and torch.equal(bits(got), bits(n2))
        assert torch.equal(bits(w1), bits(w2)) and not torch.equal(w1, torch.from_numpy(c.w).to(DEV))
