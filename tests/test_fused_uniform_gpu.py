"""The id-free (UNIFORM) body of the register-fused passes (-m gpu; csrc/stencil_fused.hip) and the census tables it is chosen
from (lmg_pattern_census): waves whose whole rectangle of rows is the hot pattern of A -- and of P / R in the transfer passes
-- never load or test a pattern id.  Everything here runs on 401 x 129 nodes (odd stride, nests to 201 x 65) and, the plain
passes, on 400 x 128, with 20-line segments: the smallest grids with at least 4 strips and 6 segments, i.e. with items that are
uniform and items that are not.

  1. the tables of A, P and R against NumPy, from the ids and the three rules, and their conservative reading;
  2. every pass against the oracle bit for bit with the body running (the host predicate says so), and against the same call
     with the switch off; the kernels built without the body (has_uniform) must report no uniform item;
  3. rows planted where an item stores, where it reads a neighbour's column or line as halo, and where only its prefetch
     reaches: same bits, and the predicate's count drops by exactly the items whose rectangle holds a planted row;
  4. a hierarchy through rebuild_numeric and back: the table and a V(3,3) cycle equal a fresh hierarchy's.

The geometry of a launch (strips, segments, the rectangle an item reads) is restated here in Python from the kernel's rules, so
that the expected counts do not come from the code under test."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rebuild_cases as RC                                           # noqa: E402
from fused_checks import check_post, check_pre, check_smoothing, jacobi_wants, nested_pair, register_pass   # noqa: E402
from learnmultigrid_amd import ops, twins                            # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy                   # noqa: E402
from oracle import kernels as K                                      # noqa: E402  (checker only)
from support import DEV, dev, nan_vec                                # noqa: E402

SEG = 20
CELL = 32


# ---- operators ---------------------------------------------------------------------------------------------------------------
def poisson_rect(Wg, Hg):
    """The 5-point Poisson operator on the Wg x Hg grid, row = y * Wg + x; boundary rows simply lack their outer entries."""
    def T(n):
        return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    A = sp.csr_matrix(sp.kron(sp.eye(Hg), T(Wg)) + sp.kron(T(Hg), sp.eye(Wg)))
    A.sort_indices()
    return K.as_csr(A)


def galerkin_rect(Wg, Hg):
    """The 9-point Galerkin operator R A P on the Wg x Hg grid, from the Poisson problem on (2 Wg - 1) x (2 Hg - 1)."""
    Pm, Rm = nested_pair(2 * Wg - 1, 2 * Hg - 1)
    A = sp.csr_matrix(Rm @ poisson_rect(2 * Wg - 1, 2 * Hg - 1) @ Pm)
    A.sort_indices()
    return K.as_csr(A)


OPERATORS = {"5pt": (poisson_rect, 0x0BA), "9pt": (galerkin_rect, 0x1FF)}
_CACHE = {}


def problem(kind, Wg, Hg):
    """(A, x0, b, oracle results of the plain passes) of an operator, computed once and never written."""
    key = (kind, Wg, Hg)
    if key not in _CACHE:
        A = OPERATORS[kind][0](Wg, Hg)
        rng = np.random.default_rng(Wg * Hg)
        x0, b = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
        _CACHE[key] = (A, x0, b, jacobi_wants(A, x0, b))
    return _CACHE[key]


def on_device(A, Wg, umask):
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack()
    S = dA.stencil
    assert S is not None and (S.W, S.umask) == (Wg, umask) and S.hot >= 0 and S.census is not None
    return dA


def transfers_on_device(Pm, Rm, Wf, Wc):
    dP, dR = ops.DeviceCSR.from_scipy(Pm, DEV), ops.DeviceCSR.from_scipy(Rm, DEV)
    dP.pack(line_strides=(Wf, Wc))
    dR.pack(line_strides=(Wf, Wc))
    assert dP.prolong is not None and dP.prolong.census is not None and dR.restrict is not None and dR.restrict.census is not None
    return dP, dR


@contextlib.contextmanager
def uniform(flag):
    try:
        ops.set_fused_uniform_enabled(flag)
        yield
    finally:
        ops.set_fused_uniform_enabled(True)


# ---- the rules, in NumPy -------------------------------------------------------------------------------------------------------
def unexpected(pid, n, W, expected):
    """bool [lines][cells * 32]: the row at (line, column) does not hold expected[2 * (line & 1) + (column & 1)]; what lies
    beyond the line stride or beyond row n - 1 is not expected either."""
    lines, cells = -(-n // W), -(-W // CELL)
    bad = np.ones((lines, cells * CELL), dtype=bool)
    i = np.arange(n)
    y, x = i // W, i % W
    bad[y, x] = pid[:n] != np.asarray(expected)[2 * (y & 1) + (x & 1)]
    return bad


def census_ref(bad):
    lines, cols = bad.shape
    table = np.zeros((lines + 1, cols // CELL + 1), dtype=np.int32)
    table[1:, 1:] = bad.reshape(lines, cols // CELL, CELL).sum(axis=2).cumsum(axis=0).cumsum(axis=1)
    return table


def expected_ids(dA, dP=None, dR=None):
    """(pid, n, W, expected) of A and, where given, of P (fine grid) and R (coarse grid)."""
    S = dA.stencil
    out = [(S.pid.cpu().numpy(), S.n, S.W, [S.hot] * 4)]
    if dP is not None:
        T = dP.prolong
        pe, po = T._hot_pairs
        out.append((T.pid.cpu().numpy(), T.n, T.W, [pe & 255, pe >> 8, po & 255, po >> 8]))
    if dR is not None:
        T = dR.restrict
        out.append((T.pid.cpu().numpy(), T.nc, T.Wc, [T.hot] * 4))
    return out


def all_expected(table, lines, W, y0, y1, x0, x1):
    """The four-load reading of a table (lmg_census_all_expected)."""
    if y0 < 0 or y1 >= lines or y0 > y1 or x0 < 0 or x1 >= W or x0 > x1:
        return False
    ca, cb = x0 // CELL, x1 // CELL + 1
    return int(table[y1 + 1, cb]) - int(table[y0, cb]) - int(table[y1 + 1, ca]) + int(table[y0, ca]) == 0


def check_table(twin_table, pid, n, W, expected, seed):
    bad = unexpected(pid, n, W, expected)
    want = census_ref(bad)
    got = twin_table.cpu().numpy().reshape(want.shape)
    assert got.dtype == np.int32 and np.array_equal(got, want), np.argwhere(got != want)[:8]
    # conservative: a rectangle read as all-expected holds no other row, and lies inside the grid
    rng = np.random.default_rng(seed)
    lines, yes = bad.shape[0], 0
    for _ in range(400):
        y0, y1 = sorted(rng.integers(-1, lines + 1, 2))
        x0, x1 = sorted(rng.integers(-2, W + 2, 2))
        if all_expected(got, lines, W, y0, y1, x0, x1):
            yes += 1
            assert 0 <= y0 <= y1 < lines and 0 <= x0 <= x1 < W and not bad[y0:y1 + 1, x0:x1 + 1].any(), (y0, y1, x0, x1)
        elif 0 <= y0 and y1 < lines and 0 <= x0 and x1 < W:
            # ... and a refusal has its reason inside the rectangle widened to whole cells
            assert bad[y0:y1 + 1, x0 // CELL * CELL:(x1 // CELL + 1) * CELL].any(), (y0, y1, x0, x1)
    return yes


# ---- the geometry of a launch, restated ----------------------------------------------------------------------------------------
def items_of(n, W, S, resid, zero, prol=False, rest=False, nc=0, Wc=0, seg_lines=SEG):
    """Every item of the launch as a dict: the strip's first window column c0, the lines it stores [out0, out1), the lines it
    reads [y_begin, y_fetch], and whether it runs the FAST body -- stencil_fused.hip's decomposition with the default tune
    keys (balanced: boundary strips and edge segments cut shorter, 55 per cent) and `seg_lines` lines per segment."""
    resid = resid or rest
    H = S + int(resid) - int(zero)
    MLmin, MRmin = (H + 1, H + 1) if rest else (H, H + 2 if prol else H)
    ML = (MLmin + 1) & ~1
    U = (128 - ML - MRmin) & ~1
    HL = H + int(rest)
    lines, strips = -(-n // W), -(-W // U)
    slow = max((seg_lines + 2 * HL) * 55 // 100 - 2 * HL, 2)
    nb, segs_b, slb, edge = 0, 1, seg_lines, 0
    if slow < seg_lines:
        nb, slb, segs_b = min(strips, 2), slow, -(-lines // slow)
        e = max(slow, HL + 2 + 6 + 2)
        if strips > nb and lines >= 2 * e + seg_lines:
            edge = e
    segs = 2 + -(-(lines - 2 * edge) // seg_lines) if edge else -(-lines // seg_lines)
    spans = [((0 if sb == 0 else strips - 1), k * slb, min(lines, (k + 1) * slb)) for sb in range(nb) for k in range(segs_b)]
    for seg in range(segs):
        if edge:
            lo, hi = ((0, edge), (lines - edge, lines))[seg] if seg < 2 else (
                edge + (seg - 2) * seg_lines, min(lines - edge, edge + (seg - 1) * seg_lines))
        else:
            lo, hi = seg * seg_lines, min(lines, (seg + 1) * seg_lines)
        spans += [(s + (1 if nb else 0), lo, hi) for s in range(strips - nb)]
    out = []
    for strip, o0, o1 in spans:
        c0 = strip * U - ML
        yb = o0 - HL - ((o0 - HL) & 1)
        t_last = o1 - 1 + S + int(resid) + int(rest)
        yf = yb + ((t_last - yb) // 6 + 1) * 6 - 1 + 2
        fast = yb >= (S + 2 if rest else 1) and yf <= lines - 2 and yb * W + c0 >= 0 and yf * W + c0 + 128 < n
        if prol:
            fast = fast and ((yf + 1) >> 1) * Wc + (c0 >> 1) + 64 <= nc
        if rest:
            fast = fast and ((yf - S) >> 1) * Wc + (c0 >> 1) + 64 <= nc
        out.append(dict(c0=c0, ML=ML, U=U, HL=HL, out0=o0, out1=o1, y_begin=yb, y_fetch=yf, fast=fast, S=S,
                        has=has_uniform(S, resid, zero)))
    return out


def has_uniform(S, resid, zero):
    """The kernels built with the UNIFORM body (kHasUniform): three sweeps, except the plain pass from a zero iterate -- in the
    others it cost registers (profiles/fused_uniform_resources.txt), and none of their items may be uniform."""
    return S == 3 and bool(resid or not zero)


def clean(bad, W, y0, y1, x0, x1):
    """No unexpected row in the rectangle widened to whole cells (False where it leaves the grid)."""
    if y0 < 0 or y1 >= bad.shape[0] or x0 < 0 or x1 >= W:
        return False
    return not bad[y0:y1 + 1, x0 // CELL * CELL:(x1 // CELL + 1) * CELL].any()


def uniform_items(items, W, badA, badP=None, badR=None, Wc=0):
    """The items that must run the UNIFORM body, from the rules alone."""
    out = []
    for it in items:
        ok = it["has"] and it["fast"] and clean(badA, W, it["y_begin"], it["y_fetch"], it["c0"], it["c0"] + 127)
        if badP is not None:
            ok = ok and clean(badP, W, it["y_begin"], it["y_fetch"], it["c0"], it["c0"] + 127)
        if badR is not None:
            S = it["S"]
            ok = ok and clean(badR, Wc, (it["y_begin"] - S) >> 1, (it["y_fetch"] - S) >> 1, it["c0"] >> 1, (it["c0"] >> 1) + 63)
        if ok:
            out.append(it)
    return out


PLAIN = [(S, resid, zero) for S in (1, 2, 3) for resid in (False, True) for zero in (False, True)]


def check_counts(dA, dP=None, dR=None):
    """The host predicate against the restated rules for every pass; returns {pass: uniform items}."""
    ids = expected_ids(dA, dP, dR)
    S_ = dA.stencil
    badA = unexpected(*ids[0])
    got = {}
    for S, resid, zero in PLAIN:
        items = items_of(S_.n, S_.W, S, resid, zero)
        want = uniform_items(items, S_.W, badA)
        g, f, u = ops.fused_uniform_items(dA, S, resid, zero)
        assert (g + f + u, g, u) == (len(items), sum(not it["fast"] for it in items), len(want)), (S, resid, zero, g, f, u)
        got["plain", S, resid, zero] = want
    if dP is not None:
        T = dP.prolong
        badP = unexpected(*ids[1])
        for S in (1, 2, 3):
            items = items_of(S_.n, S_.W, S, False, False, prol=True, nc=T.nc, Wc=T.Wc)
            want = uniform_items(items, S_.W, badA, badP=badP)
            g, f, u = ops.fused_uniform_items(dA, S, prolong=dP)
            assert (g + f + u, u) == (len(items), len(want)), ("prolong", S, g, f, u)
            got["prolong", S] = want
    if dR is not None:
        T = dR.restrict
        badR = unexpected(*ids[-1])
        for S in (1, 2, 3):
            for zero in (False, True):
                items = items_of(S_.n, S_.W, S, True, zero, rest=True, nc=T.nc, Wc=T.Wc)
                want = uniform_items(items, S_.W, badA, badR=badR, Wc=T.Wc)
                g, f, u = ops.fused_uniform_items(dA, S, zero=zero, restrict=dR)
                assert (g + f + u, u) == (len(items), len(want)), ("restrict", S, zero, g, f, u)
                got["restrict", S, zero] = want
    return got


# ---- 1. the census -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(OPERATORS))
def test_census_tables_against_numpy(kind):
    A = problem(kind, 401, 129)[0]
    dA = on_device(A, 401, OPERATORS[kind][1])
    Pm, Rm = nested_pair(401, 129)
    dP, dR = transfers_on_device(Pm, Rm, 401, 201)
    tables = (dA.stencil.census, dP.prolong.census, dR.restrict.census)
    for k, (table, ids) in enumerate(zip(tables, expected_ids(dA, dP, dR))):
        assert table.numel() == (ids[1] // ids[2] + 1) * twins.census_stride(ids[2])
        yes = check_table(table, *ids, seed=k)
        assert yes > 20, (kind, k, yes)                         # (the random rectangles do meet clean ones)


def test_census_of_a_ragged_grid_with_four_expected_ids():
    """61 lines of 70 less 13 rows, ids 0..3 by parity with 2 per cent strays: the short last line and the columns of the last
    cell beyond the stride count, and the four parities are told apart."""
    n, W = 61 * 70 - 13, 70
    rng = np.random.default_rng(70)
    i = np.arange(n)
    pid = (2 * ((i // W) & 1) + ((i % W) & 1)).astype(np.uint8)
    stray = rng.random(n) < 0.02
    pid[stray] = rng.integers(0, 6, int(stray.sum()))
    table = twins.census_table(dev(pid), n, W, [0, 1, 2, 3])
    assert check_table(table, pid, n, W, [0, 1, 2, 3], seed=5) > 0
    assert twins.census_table(dev(pid), n, W, [0, 1, -1, 3]) is None


# ---- 2. parity with the body running -------------------------------------------------------------------------------------------
def plain_results(dA, x0, b):
    n = dA.shape[0]
    out = []
    for omega in (0.8, 1.0):
        for S, resid, zero in PLAIN:
            x, r = nan_vec(n), (nan_vec(n) if resid else None)
            ops.stencil_smooth(dA, None if zero else dev(x0), dev(b), omega, S, x, r)
            out += [x.cpu().numpy()] + ([r.cpu().numpy()] if resid else [])
    return out


def transfer_results(dA, dP, dR, x0, b, e):
    n, nc = dA.shape[0], dP.shape[1]
    out = []
    for S in (1, 2, 3):
        x = nan_vec(n)
        ops.stencil_smooth(dA, dev(x0), dev(b), 0.8, S, x, None, prolong=(dP, dev(e)))
        out.append(x.cpu().numpy())
        for zero in (False, True):
            x, bc = nan_vec(n), nan_vec(nc)
            ops.stencil_smooth(dA, None if zero else dev(x0), dev(b), 0.8, S, x, None, restrict=(dR, bc))
            out += [x.cpu().numpy(), bc.cpu().numpy()]
    return out


def same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert not np.isnan(g).any() and np.array_equal(g, w), (k, np.flatnonzero(g != w)[:8])


@pytest.mark.parametrize("Wg,Hg", [(401, 129), (400, 128)])
@pytest.mark.parametrize("kind", sorted(OPERATORS))
def test_passes_with_uniform_items_equal_the_oracle_and_the_switch_off(kind, Wg, Hg):
    A, x0, b, wants = problem(kind, Wg, Hg)
    dA = on_device(A, Wg, OPERATORS[kind][1])
    with register_pass(SEG):
        assert ops._fused_kind(dA) is None
        counts = check_counts(dA)
        for key, uni in counts.items():
            items = ops.fused_uniform_items(dA, *key[1:])
            if has_uniform(*key[1:]):
                assert len(uni) > 0 and items[0] + items[1] > 0, (key, items)         # some are uniform, some are not
            else:
                assert len(uni) == 0 and items[2] == 0, (key, items)                  # a kernel without the body
        check_smoothing((kind, Wg, Hg), dA, x0, b, wants)
        on = plain_results(dA, x0, b)
        with uniform(False):
            assert ops.fused_uniform_items(dA, 3, True)[2] == 0
            same(on, plain_results(dA, x0, b))


@pytest.mark.parametrize("kind", sorted(OPERATORS))
def test_transfer_passes_with_uniform_items_equal_the_oracle_and_the_switch_off(kind):
    Wg, Hg = 401, 129
    A, x0, b, _ = problem(kind, Wg, Hg)
    Pm, Rm = nested_pair(Wg, Hg)
    dA = on_device(A, Wg, OPERATORS[kind][1])
    dP, dR = transfers_on_device(Pm, Rm, Wg, 201)
    e = np.random.default_rng(201).standard_normal(Pm.shape[1])
    with register_pass(SEG):
        counts = check_counts(dA, dP, dR)
        for k in (k for k in counts if k[0] in ("prolong", "restrict")):      # (never all: the edges are not FAST)
            assert (len(counts[k]) > 0) == (k[1] == 3), k
        check_pre(A, Rm, dA, dR, x0, b)
        check_post(A, Pm, dA, dP, x0, b, e)
        on = transfer_results(dA, dP, dR, x0, b, e)
        with uniform(False):
            assert ops.fused_uniform_items(dA, 3, restrict=dR)[2] == 0 and ops.fused_uniform_items(dA, 3, prolong=dP)[2] == 0
            same(on, transfer_results(dA, dP, dR, x0, b, e))


# ---- 3. planted exceptions -----------------------------------------------------------------------------------------------------
def plant(A, rows):
    """A with one off-diagonal value of each of `rows` scaled by its own factor: every one becomes a pattern of its own."""
    B = A.copy()
    for k, i in enumerate(rows):
        j = B.indptr[i]                                              # the first entry of an interior row: off the diagonal
        assert B.indices[j] != i
        B.data[j] *= 1.5 + 0.25 * k
    return K.as_csr(B)


@pytest.mark.parametrize("kind", sorted(OPERATORS))
def test_planted_rows_keep_the_bits_and_cost_exactly_their_items(kind):
    Wg, Hg = 401, 129
    A, x0, b, _ = problem(kind, Wg, Hg)
    n = A.shape[0]
    # places, from the geometry of the restricting pass of three sweeps: a uniform item `it` of the second strip ...
    geo = items_of(n, Wg, 3, True, False, rest=True, nc=201 * 65, Wc=201)
    badA0 = unexpected(*expected_ids(on_device(A, Wg, OPERATORS[kind][1]))[0])
    uni0 = uniform_items(geo, Wg, badA0)
    it = next(i for i in uni0 if i["c0"] > 128 and any(j["c0"] == i["c0"] and j["out0"] == i["out1"] for j in uni0))
    left = next(i for i in uni0 if i["c0"] == it["c0"] - it["U"] and i["out0"] == it["out0"])
    places = {
        "stored": (it["out0"] + 3, it["c0"] + it["ML"] + 10),
        # stored by the strip on the left, inside this strip's left margin
        "halo column": (it["out0"] + 5, it["c0"] + 1),
        # the first line of the next segment: stored there, read here as halo
        "halo line": (it["out1"], it["c0"] + it["ML"] + 40),
        # a line this item only prefetches: it computes nothing from it
        "prefetch only": (it["y_fetch"], it["c0"] + it["ML"] + 70),
    }
    assert left["c0"] + left["ML"] <= places["halo column"][1] < left["c0"] + left["ML"] + left["U"]
    assert places["prefetch only"][0] >= it["out1"] + it["HL"] + 1
    rows = [y * Wg + x for y, x in places.values()]
    B = plant(A, rows)
    Pm, _ = nested_pair(Wg, Hg)
    Pm = sp.csr_matrix(Pm)
    yp, xp = 2 * 31 + 1, 2 * 70 + 1                                  # an odd-odd fine node: four entries, all interior
    j = Pm.indptr[yp * Wg + xp]
    assert Pm.indptr[yp * Wg + xp + 1] - j == 4
    Pm.data[j + 2] *= 1.25
    Pm = K.as_csr(Pm)
    Rm = K.as_csr(sp.csr_matrix(Pm.T))
    dA0 = on_device(A, Wg, OPERATORS[kind][1])
    dB = on_device(B, Wg, OPERATORS[kind][1])
    assert dB.stencil.npat == dA0.stencil.npat + 4
    dP0, dR0 = transfers_on_device(*nested_pair(Wg, Hg), Wg, 201)
    dP, dR = transfers_on_device(Pm, Rm, Wg, 201)
    e = np.random.default_rng(7).standard_normal(Pm.shape[1])
    with register_pass(SEG):
        before = check_counts(dA0, dP0, dR0)
        after = check_counts(dB, dP, dR)                             # (each count against the restated rules)
        ids0, ids1 = expected_ids(dA0, dP0, dR0), expected_ids(dB, dP, dR)
        planted = [unexpected(*a) ^ unexpected(*c) for a, c in zip(ids0, ids1)]
        assert planted[0].sum() == 4 and planted[1].sum() == 1 and planted[2].sum() >= 1
        for key in before:
            lost = [i for i in before[key] if i not in after[key]]
            has = has_uniform(*{"plain": key[1:], "prolong": (key[1], False, False), "restrict": (key[1], True, key[-1])}[key[0]])
            assert not [i for i in after[key] if i not in before[key]] and (len(after[key]) > 0) == has, key
            # exactly the items whose rectangle (in cells) holds a planted row
            S_ = key[1]
            hit = []
            for i in before[key]:
                h = not clean(planted[0], Wg, i["y_begin"], i["y_fetch"], i["c0"], i["c0"] + 127)
                if key[0] == "prolong":
                    h = h or not clean(planted[1], Wg, i["y_begin"], i["y_fetch"], i["c0"], i["c0"] + 127)
                if key[0] == "restrict":
                    h = h or not clean(planted[2], 201, (i["y_begin"] - S_) >> 1, (i["y_fetch"] - S_) >> 1, i["c0"] >> 1,
                                       (i["c0"] >> 1) + 63)
                if h:
                    hit.append(i)
            assert lost == hit and (len(hit) > 0) == has, (key, len(lost), len(hit))
        assert it in before["restrict", 3, False] and it not in after["restrict", 3, False]
        wants = jacobi_wants(B, x0, b)
        check_smoothing((kind, "planted"), dB, x0, b, wants)
        check_pre(B, Rm, dB, dR, x0, b)
        check_post(B, Pm, dB, dP, x0, b, e)


# ---- 4. staleness --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Wg,Hg", [(401, 129), (129, 129)])
def test_rebuild_numeric_takes_the_census_along(Wg, Hg):
    """401 x 129: items on the UNIFORM body.  129^2: too narrow for one, but a square grid, on which the hierarchy's own
    pack() finds the window twins of P and R: their tables are compared as well."""
    A = poisson_rect(Wg, Hg)
    hier = [sp.csr_matrix(nested_pair(Wg, Hg)[0]), sp.csr_matrix(nested_pair((Wg + 1) // 2, (Hg + 1) // 2)[0])]
    B = plant(A, [60 * Wg + Wg // 2])
    square, some = Wg == Hg, (lambda u: u > 0) if Wg > 256 else (lambda u: u == 0)
    rhs = RC.rhs(A.shape[0], seed=11)
    saved = ops.FUSED_MIN_ROWS, ops.FUSED_TRANSFER_MIN_ROWS

    def cycle(H):
        with torch.cuda.stream(H.stream):
            H.levels[0].b.copy_(dev(rhs))
            H.cycle("Jacobi", 3, 0.8, x_is_zero=True)
            x = H.levels[0].x.clone()
        torch.cuda.synchronize()
        return x

    def fresh(M):
        F = Hierarchy(M.copy(), list(hier), DEV)
        torch.cuda.synchronize()
        return F

    try:
        ops.FUSED_MIN_ROWS = ops.FUSED_TRANSFER_MIN_ROWS = 0          # every level on the register pass
        with register_pass(SEG):
            H, F0, F1 = fresh(A), fresh(A), fresh(B)
            assert ops._fused_kind(H.levels[0].A) == "reg" and some(ops.fused_uniform_items(H.levels[0].A, 3)[2])
            assert (H.levels[0].P.prolong is not None and H.levels[0].R.restrict is not None) == square
            x0 = cycle(H)
            assert torch.equal(x0, cycle(F0))
            for M, F in ((B, F1), (A, F0), (B, F1)):
                with torch.cuda.stream(H.stream):
                    H.rebuild_numeric(RC.values(M).to(DEV))
                torch.cuda.synchronize()
                got, want = H.levels[0].A.stencil, F.levels[0].A.stencil
                assert got.census is not None and got.hot == want.hot and torch.equal(got.census, want.census)
                assert ops.fused_uniform_items(H.levels[0].A, 3) == ops.fused_uniform_items(F.levels[0].A, 3)
                for h, f in zip(H.levels[:-1], F.levels[:-1]):                  # the tables of the transfers and of every level
                    for Mh, Mf, form in ((h.A, f.A, "stencil"), (h.P, f.P, "prolong"), (h.R, f.R, "restrict")):
                        th, tf = getattr(Mh, form), getattr(Mf, form)
                        assert (th is None) == (tf is None), (h.n, form)
                        if th is not None:
                            assert (th.census is None) == (tf.census is None), (h.n, form)
                            assert th.census is None or torch.equal(th.census, tf.census), (h.n, form)
                if square:
                    assert H.levels[0].P.prolong.census is not None and H.levels[0].R.restrict.census is not None
                assert torch.equal(cycle(H), cycle(F))
            assert not torch.equal(F0.levels[0].A.stencil.census, F1.levels[0].A.stencil.census)
            if not square:
                assert ops.fused_uniform_items(F1.levels[0].A, 3)[2] < ops.fused_uniform_items(F0.levels[0].A, 3)[2]
    finally:
        ops.FUSED_MIN_ROWS, ops.FUSED_TRANSFER_MIN_ROWS = saved
