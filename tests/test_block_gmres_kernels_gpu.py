"""The block Gram-Schmidt kernels of block GMRES (csrc/krylov.hip) on the device (-m gpu), bit for bit against the
single-vector kernels run on contiguous copies of each column: lmg_block_multi_dot against ops.multi_dot,
lmg_block_multi_axpy (unequal counts per column, both signs, with and without the norm) against ops.multi_axpy,
lmg_block_scale against ops.axpby; the slack of a basis with ldb > n k and the bytes of a column with a count of 0 are never
written; the argument checks of the three entry points and of their wrappers.

Shapes: k = 2, 4, 8; n = 1, 2 (no pair / one pair), 255 (less than a workgroup), 1089 (odd, several workgroups) and
524288 + 515 (odd, a partly filled second trip of the 1024 x 256 grid-stride over row pairs); nb = 1, C, C + 1, 2 C + 1
around the C = 32 / k blocks one lane of the dot kernel keeps in registers; ldb = n k + 6 with NaN in the slack."""
import ctypes
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from learnmultigrid_amd import _lib, ops   # noqa: E402
from support import DEV                    # noqa: E402

F64 = torch.float64
KS = (2, 4, 8)
NS = (1, 2, 255, 1089, 524288 + 515)
SLACK = 6
NAN = float("nan")


def chunk(k):
    return 32 // k


def bits(t):
    return t.contiguous().view(torch.int64)


def spread(gen, size):
    """Entries over 1e-8 .. 1e+8 with random signs: a summation-order mistake moves the result far beyond rounding."""
    mag = 10.0 ** (16.0 * torch.rand(size, dtype=F64, device=DEV, generator=gen) - 8.0)
    return torch.where(torch.rand(size, dtype=F64, device=DEV, generator=gen) < 0.5, -mag, mag)


class Case:
    """A basis of nbmax = 2 C + 1 blocks with ldb = n k + SLACK and a block W, NaN in every slack; flat / flat_w are the
    allocations the C ABI sees, Vb (nbmax, n, k) a contiguous copy for the wrappers, W0 the values of W."""

    def __init__(self, k, n):
        self.k, self.n = k, n
        self.nbmax = 2 * chunk(k) + 1
        self.ldb = n * k + SLACK
        gen = torch.Generator(device=DEV)
        gen.manual_seed(1000 * k + n % 997)
        self.flat = torch.full((self.nbmax * self.ldb,), NAN, dtype=F64, device=DEV)
        rows = self.flat.view(self.nbmax, self.ldb)
        rows[:, :n * k] = spread(gen, (self.nbmax, n * k))
        self.flat_bits = bits(self.flat).clone()
        self.Vb = rows[:, :n * k].reshape(self.nbmax, n, k).clone()
        self.W0 = spread(gen, (n, k))
        self.coef = spread(gen, (self.nbmax * k,)) * 1e-4

    def w(self, values=None):
        """A fresh W = values (W0) at the start of an allocation with NaN behind it: (flat_w, W)."""
        flat_w = torch.full((self.n * self.k + SLACK,), NAN, dtype=F64, device=DEV)
        W = flat_w[:self.n * self.k].view(self.n, self.k)
        W.copy_(self.W0 if values is None else values)
        return flat_w, W

    def column_basis(self, V, j, rows):
        """Column j of the first `rows` blocks of V (nb, n, k) as a contiguous single-vector basis (rows, ldv), ldv even."""
        ldv = self.n + (self.n & 1)
        Vc = torch.zeros((max(rows, 1), ldv), dtype=F64, device=DEV)
        Vc[:rows, :self.n] = V[:rows, :, j]
        return Vc

    def untouched(self, flat_w=None):
        assert torch.equal(bits(self.flat), self.flat_bits)
        if flat_w is not None:
            assert bool(torch.isnan(flat_w[self.n * self.k:]).all())


@functools.lru_cache(maxsize=2)
def case(k, n):
    return Case(k, n)


def lib():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


GRID = [(k, n) for k in KS for n in NS]


# ---- block_multi_dot ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", GRID)
def test_block_multi_dot_has_the_bits_of_multi_dot_on_every_column(k, n):
    c = case(k, n)
    C = chunk(k)
    flat_w, W = c.w()
    part1 = torch.empty(ops.multi_partials_count(n, c.nbmax), dtype=F64, device=DEV)
    want = torch.empty((c.nbmax, k), dtype=F64, device=DEV)
    for j in range(k):
        col = torch.empty(c.nbmax, dtype=F64, device=DEV)
        ops.multi_dot(c.column_basis(c.Vb, j, c.nbmax), c.nbmax, W[:, j].clone(), part1, col)
        want[:, j] = col
    assert bool(torch.isfinite(want).all())
    for nb in (1, C, C + 1, 2 * C + 1):
        assert lib().lmg_block_multi_partials_count(n, k, nb) == 1024 * k * nb
        part = torch.full((ops.block_multi_partials_count(n, k, nb),), 123.0, dtype=F64, device=DEV)
        out = torch.full((c.nbmax * k + 1,), NAN, dtype=F64, device=DEV)
        rc = lib().lmg_block_multi_dot(k, n, nb, c.flat.data_ptr(), c.ldb, W.data_ptr(), part.data_ptr(), out.data_ptr(), stream())
        assert rc == 0
        assert torch.equal(bits(out[:nb * k]), bits(want[:nb].reshape(-1))), nb          # row i's bits do not depend on nb
        assert bool(torch.isnan(out[nb * k:]).all())
    # the wrapper on the contiguous copy (ldb = n k): the same bits
    out2 = torch.full((c.nbmax * k,), NAN, dtype=F64, device=DEV)
    ops.block_multi_dot(c.Vb, c.nbmax, W, part, out2)
    assert torch.equal(bits(out2), bits(want.reshape(-1)))
    c.untouched(flat_w)
    assert torch.equal(bits(W), bits(c.W0))


# ---- block_multi_axpy ---------------------------------------------------------------------------------------------------------
def counts_for(k, nbmax, C, variant):
    base = [0, nbmax, C, C + 1, 1, 0, 2 * C, 3]
    if variant:
        base = [C + 1, 0, 1, nbmax, 2, 0, 0, C]
    return [min(v, nbmax) for v in base[:k]]


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("k,n", GRID)
def test_block_multi_axpy_has_the_bits_of_multi_axpy_on_every_column(k, n, variant):
    c = case(k, n)
    counts = counts_for(k, c.nbmax, chunk(k), variant)
    assert 0 in counts and len(set(counts)) > 1
    nbuse = max(counts)
    # blocks a column does not reach hold NaN in that column: reading one would show
    flatV = c.flat.clone()
    Vrows = flatV.view(c.nbmax, c.ldb)[:, :n * k]
    V3 = c.Vb.clone()
    for j in range(k):
        V3[counts[j]:, :, j] = NAN
    Vrows.copy_(V3.reshape(c.nbmax, n * k))
    part1 = torch.empty(ops.multi_partials_count(n, c.nbmax), dtype=F64, device=DEV)
    part = torch.full((ops.block_multi_partials_count(n, k, 1),), 123.0, dtype=F64, device=DEV)
    h_counts = (ctypes.c_int * k)(*counts)
    for subtract in (True, False):
        want = torch.empty((n, k), dtype=F64, device=DEV)
        want2 = torch.empty(k, dtype=F64, device=DEV)
        for j in range(k):
            wj = c.W0[:, j].clone()
            n2 = torch.zeros(1, dtype=F64, device=DEV)
            ops.multi_axpy(c.column_basis(V3, j, counts[j]), counts[j], c.coef[j::k][:max(counts[j], 1)].clone(), wj, part1, n2,
                           subtract=subtract)
            want[:, j] = wj
            want2[j:j + 1] = n2
        assert bool(torch.isfinite(want).all())
        for with_norm in (True, False):
            flat_w, W = c.w()
            norm2 = torch.full((k + 1,), NAN, dtype=F64, device=DEV)
            part.fill_(123.0)
            rc = lib().lmg_block_multi_axpy(k, n, h_counts, 1 if subtract else 0, flatV.data_ptr(), c.ldb, c.coef.data_ptr(),
                                            W.data_ptr(), part.data_ptr(), norm2.data_ptr() if with_norm else None, stream())
            assert rc == 0
            assert torch.equal(bits(W), bits(want)), (subtract, with_norm)
            for j in range(k):
                assert (counts[j] == 0) == torch.equal(bits(W[:, j]), bits(c.W0[:, j])), j
            assert bool(torch.isnan(flat_w[n * k:]).all())
            if with_norm:
                assert torch.equal(bits(norm2[:k]), bits(want2)) and bool(torch.isnan(norm2[k:]).all())
            else:
                assert bool((part == 123.0).all())                      # without the norm the scratch is not written
        # the wrapper on the contiguous copy, coefficients and counts the same
        _, W = c.w()
        norm2 = torch.zeros(k, dtype=F64, device=DEV)
        ops.block_multi_axpy(V3, counts, c.coef, W, part, norm2, subtract=subtract)
        assert torch.equal(bits(W), bits(want)) and torch.equal(bits(norm2), bits(want2))
    assert nbuse <= c.nbmax
    after = flatV.view(c.nbmax, c.ldb)
    assert bool(torch.isnan(after[:, n * k:]).all()) and torch.equal(bits(after[:, :n * k]), bits(V3.reshape(c.nbmax, n * k)))
    c.untouched()


@pytest.mark.parametrize("k,n", [(k, n) for k in KS for n in (1, 2, 1089)])
def test_a_column_with_count_zero_keeps_its_bytes(k, n):
    """The columns that are off hold NaNs with a payload (and an Inf): compared as raw bytes they are unchanged, their norm2
    is that of their contents (NaN), and the columns that are on are not touched by them."""
    c = case(k, n)
    counts = [0 if j % 2 == 0 else 2 for j in range(k)]
    payload = torch.tensor([0x7FF8DEADBEEF0001], dtype=torch.int64, device=DEV).view(F64)
    start = c.W0.clone()
    for j in range(0, k, 2):
        start[:, j] = payload
        if n > 1:
            start[0, j] = float("inf")
    flat_w, W = c.w(start)
    before = bits(W).clone()
    part = torch.empty(ops.block_multi_partials_count(n, k, 1), dtype=F64, device=DEV)
    norm2 = torch.zeros(k, dtype=F64, device=DEV)
    ops.block_multi_axpy(c.Vb, counts, c.coef, W, part, norm2)
    after = bits(W)
    part1 = torch.empty(ops.multi_partials_count(n, 2), dtype=F64, device=DEV)
    for j in range(k):
        if counts[j] == 0:
            assert torch.equal(after[:, j], before[:, j])               # raw bytes: payload and sign of every NaN
            assert bool(torch.isnan(norm2[j]))
        else:
            wj = c.W0[:, j].clone()
            n2 = torch.zeros(1, dtype=F64, device=DEV)
            ops.multi_axpy(c.column_basis(c.Vb, j, 2), 2, c.coef[j::k][:2].clone(), wj, part1, n2)
            assert torch.equal(bits(W[:, j]), bits(wj)) and torch.equal(bits(norm2[j:j + 1]), bits(n2))
    assert bool(torch.isnan(flat_w[n * k:]).all())
    # every column off, no norm: nothing is launched, nothing changes
    ops.block_multi_axpy(c.Vb, [0] * k, c.coef, W)
    assert torch.equal(bits(W), after)
    # every column off with the norm: the norms of the contents, finite columns with multi_axpy's bits
    ops.block_multi_axpy(c.Vb, [0] * k, c.coef, W, part, norm2)
    assert torch.equal(bits(W), after)
    for j in range(1, k, 2):
        wj = W[:, j].clone()
        n2 = torch.zeros(1, dtype=F64, device=DEV)
        ops.multi_axpy(c.column_basis(c.Vb, j, 0), 0, c.coef[:1], wj, part1, n2)
        assert torch.equal(bits(norm2[j:j + 1]), bits(n2))


# ---- block_scale --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", GRID)
def test_block_scale_has_the_bits_of_axpby_and_empties_a_column(k, n):
    c = case(k, n)
    start = c.W0.clone()
    start[:, 1] = NAN
    start[0, 1] = float("inf")
    start[n - 1, 1] = -float("inf")
    scale = [1.0 / 3.0, 0.0, -7.25e-3, 1.0, 0.0, 1e300, 3.0, -1.0][:k]
    flat_w, W = c.w(start)
    ops.block_scale(scale, W)
    for j in range(k):
        if scale[j] == 0.0:
            assert not bool(bits(W[:, j]).any())                        # +0.0, whatever the column held
        else:
            wj = start[:, j].clone()
            ops.axpby(scale[j], wj, 0.0, wj)
            assert torch.equal(bits(W[:, j]), bits(wj)), j
    assert bool(torch.isnan(flat_w[n * k:]).all())


# ---- argument checks ----------------------------------------------------------------------------------------------------------
def test_argument_checks():
    L = lib()
    kmax = L.lmg_krylov_max_vectors()
    ARG, ALIGN = -1, -2
    n, nb = 100, 3
    for k in KS:
        ldb = n * k
        V = torch.ones(nb * ldb + 2, dtype=F64, device=DEV)
        W = torch.ones(n * k + 2, dtype=F64, device=DEV)
        part = torch.zeros(L.lmg_block_multi_partials_count(n, k, kmax), dtype=F64, device=DEV)
        out = torch.full((kmax * k,), NAN, dtype=F64, device=DEV)
        pV, pW, pp, po = V.data_ptr(), W.data_ptr(), part.data_ptr(), out.data_ptr()

        def dot(k=k, n=n, nb=nb, V=pV, ldb=ldb, W=pW, part=pp, out=po):
            return L.lmg_block_multi_dot(k, n, nb, V, ldb, W, part, out, None)

        def axpy(k=k, n=n, counts=(nb,) * 8, V=pV, ldb=ldb, coef=po, W=pW, part=pp, norm2=po + 8 * (kmax * k - k)):
            h = None if counts is None else (ctypes.c_int * 8)(*counts)
            return L.lmg_block_multi_axpy(k, n, h, 1, V, ldb, coef, W, part, norm2, None)

        def scale(k=k, n=n, s=(2.0,) * 8, W=pW):
            h = None if s is None else (ctypes.c_double * 8)(*s)
            return L.lmg_block_scale(k, n, h, W, None)

        for bad in (0, 1, 3, 5, 6, 7, 16, -2):
            assert dot(k=bad) == ARG and axpy(k=bad) == ARG and scale(k=bad) == ARG
        for call in (dot, axpy):
            assert call(V=None) == ARG and call(W=None) == ARG and call(n=-1) == ARG
            assert call(ldb=ldb - 2) == ARG                              # < n k
            assert call(ldb=ldb + 1) == ARG                              # odd
            assert call(V=pV + 8) == ALIGN and call(W=pW + 8) == ALIGN
        assert dot(nb=-1) == ARG and dot(nb=kmax + 1) == ARG and dot(out=None) == ARG and dot(part=None) == ARG
        assert axpy(counts=None) == ARG and axpy(coef=None) == ARG and axpy(part=None) == ARG
        assert axpy(counts=(1, -1) * 4) == ARG and axpy(counts=(kmax + 1, 0) * 4) == ARG
        assert scale(s=None) == ARG and scale(W=None) == ARG and scale(n=-1) == ARG and scale(W=pW + 8) == ALIGN
        torch.cuda.synchronize()
        assert bool((V == 1.0).all()) and bool((W == 1.0).all()) and bool(torch.isnan(out).all())
        # nothing to do
        assert dot(nb=0, V=None, W=None, part=None, out=None) == 0
        assert dot(n=0, V=None, W=None) == 0
        assert axpy(n=0, V=None, W=None, part=None, norm2=None) == 0
        assert axpy(counts=(0,) * 8, V=None, coef=None, part=None, norm2=None) == 0
        assert scale(n=0, W=None) == 0
        torch.cuda.synchronize()
        assert not out[:nb * k].cpu().numpy().any() and bool(torch.isnan(out[nb * k:]).all())      # n == 0: the dots are 0
        assert bool((W == 1.0).all())
    # the wrappers refuse what the C ABI cannot see
    k = 4
    V = torch.ones((3, n, k), dtype=F64, device=DEV)
    W = torch.ones((n, k), dtype=F64, device=DEV)
    part = torch.zeros(ops.block_multi_partials_count(n, k, 3), dtype=F64, device=DEV)
    out = torch.zeros(3 * k, dtype=F64, device=DEV)
    with pytest.raises(ValueError):
        ops.block_multi_dot(V, 4, W, part, out)                          # more blocks than the basis has
    with pytest.raises(ValueError):
        ops.block_multi_dot(V, 3, W, part, out[:3 * k - 1])
    with pytest.raises(ValueError):
        ops.block_multi_dot(V, 3, torch.ones((n, 8), dtype=F64, device=DEV), part, out)
    with pytest.raises(ValueError):
        ops.block_multi_dot(V, 3, torch.ones((n, 3), dtype=F64, device=DEV), part, out)
    with pytest.raises(ValueError):
        ops.block_multi_dot(V[:, :, :2].clone(), 3, W, part, out)
    with pytest.raises(ValueError):
        ops.block_multi_axpy(V, [1, 1, 1], out, W)                       # k counts
    with pytest.raises(ValueError):
        ops.block_multi_axpy(V, [1, 4, 1, 1], out, W)                    # a count beyond the basis
    with pytest.raises(ValueError):
        ops.block_multi_axpy(V, [1, -1, 1, 1], out, W)
    with pytest.raises(ValueError):
        ops.block_multi_axpy(V, [3, 3, 3, 3], out, W, None, out)         # a norm without partials
    with pytest.raises(ValueError):
        ops.block_scale([1.0, 2.0], W)
    with pytest.raises(ValueError):
        ops.block_scale([1.0] * 4, torch.ones(4 * n + 1, dtype=F64, device=DEV)[1:].view(n, k))      # off 16 bytes
    assert bool((W == 1.0).all())
