"""CPU-only checks of the decisions twins.py takes on a verified pattern table: the window slots of every pattern, the
line stride, the hot patterns, and what is refused.

The pattern table of a SciPy matrix is built here with NumPy (pattern_table), the expected answers come from how the
matrix was constructed, and a decoded twin is checked by rebuilding the matrix from (ids, values, masks, stride) and
comparing it with the input entry for entry.  The stencil and restriction cases run twice: through the plain functions,
and through StencilTwin / RestrictTwin.from_patterns on a stand-in RowPatterns record with CPU tensors (possible wherever
one hot-pattern candidate exists, so that no device histogram is asked for).  ProlongTwin.from_patterns always counts on
the device: its decisions are checked through the functions, with the counts of np.bincount."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from learnmultigrid_amd import _lib, ops, problems, twins


def pattern_table(A, grid_map=None):
    """(pid, ptr, off, val): the distinct rows of A -- column - base(row) and the value bits of every entry -- in
    first-seen order, and a uint8 id per row."""
    base = ops.RowPatterns.grid_base(grid_map, np.arange(A.shape[0], dtype=np.int64))
    seen, pid, ptr, off, val = {}, [], [0], [], []
    for i in range(A.shape[0]):
        row = slice(A.indptr[i], A.indptr[i + 1])
        o = A.indices[row].astype(np.int64) - base[i]
        key = (o.tobytes(), A.data[row].tobytes())
        if key not in seen:
            seen[key] = len(seen)
            off += list(o)
            val += list(A.data[row])
            ptr.append(len(off))
        pid.append(seen[key])
    return np.array(pid, np.uint8), np.array(ptr, np.int32), np.array(off, np.int64), np.array(val, np.float64)


def record(A, grid_map=None):
    """What from_patterns reads of a RowPatterns twin, on the CPU."""
    pid, ptr, off, val = pattern_table(A, grid_map)
    return SimpleNamespace(n=A.shape[0], npat=len(ptr) - 1, nent=len(off), grid_map=grid_map, pid=torch.from_numpy(pid),
                           pat_ptr=torch.from_numpy(ptr), pat_off=torch.from_numpy(off.astype(np.int32)),
                           pat_val=torch.from_numpy(val))


def assert_rebuilds(A, pid, values, mask, window, grid_map=None):
    """Row i of A has exactly the entries values[pid[i] * k + q] at column base(i) + window[q], q a bit of mask[pid[i]]."""
    k = len(window)
    base = ops.RowPatterns.grid_base(grid_map, np.arange(A.shape[0], dtype=np.int64))
    ent = [(i, base[i] + window[q], values[p * k + q]) for i, p in enumerate(pid) for q in range(k) if mask[p] >> q & 1]
    rows, cols, vals = (np.array(v) for v in zip(*ent))
    B = sp.csr_matrix((vals, (rows, cols)), shape=A.shape)
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)


def window_3x3(W):
    return [c * W + d for c in (-1, 0, 1) for d in (-1, 0, 1)]


def csr(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    return A


def banded(n, offsets, values):
    return csr(sp.diags(values, offsets, shape=(n, n)))


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


# ---- square operators -----------------------------------------------------------------------------------------------------
def stencil_by_functions(A):
    """(W, values, mask, ids, hot = None: the candidates are from_patterns' business) or None."""
    pid, ptr, off, val = pattern_table(A)
    W = twins.line_stride(off, A.shape[0])
    dec = None if W is None else twins.decode_window(ptr, off, val, 9, twins.slot_3x3(W))
    return None if dec is None else (W, dec[0], dec[1], pid, None)


def stencil_by_twin(A):
    R = record(A)
    S = ops.StencilTwin.from_patterns(R, A.shape)
    if S is None:
        return None
    assert S.pid is R.pid and S.patterns is R and (S.n, S.npat) == (R.n, R.npat) and S.bytes() == R.n + 76 * R.npat
    assert S.st_val.dtype == torch.float64 and S.st_mask.dtype == torch.int32
    mask = S.st_mask.numpy()
    assert S.umask == np.bitwise_or.reduce(mask)
    if S.hot < 0:                          # no pattern has every union slot (x-periodic 5-point: interior and wrap-around rows)
        assert S.hot == -1 and S._hot_val is None
    else:
        assert list(S._hot_val) == list(S.st_val.numpy()[S.hot * 9: S.hot * 9 + 9])
    assert S.c_args()[:2] + S.c_args()[6:8] == (S.n, S.W, S.umask, S.hot)
    return S.W, S.st_val.numpy(), mask, R.pid.numpy(), S.hot


STENCIL = {"functions": stencil_by_functions, "from_patterns": stencil_by_twin}


@pytest.fixture(params=sorted(STENCIL))
def stencil_of(request):
    """Both routes to a stencil view; only from_patterns needs the library (it asks it for the pattern limit)."""
    if request.param == "from_patterns":
        request.getfixturevalue("L")
    return STENCIL[request.param]


def square_cases():
    """name -> (A, W, union mask, an interior row): what the construction of each matrix dictates."""
    out = {}
    for m in (3, 5, 6):
        out["poisson%d" % m] = (csr(problems.poisson_2d_structured(m)[0]), m + 1, 0x0BA, m + 2)
    # the 9-point Galerkin operator of the 17 x 17 problem on the 9 x 9 grid; all nine slots two nodes off the boundary
    A, P = problems.poisson_2d_structured(16)[0], problems.tensor_interpolator_2d(17)
    out["galerkin"] = (csr(P.T @ A @ P), 9, 0x1FF, 4 * 9 + 4)
    # 5 lines of 7 columns, the last line cut short: 31 rows, which none of the candidate strides 6, 7, 8 divides
    out["cut_grid"] = (banded(31, [-7, -1, 0, 1, 7], [-1.0, -1.0, 4.0, -1.0, -1.0]), 7, 0x0BA, 15)
    out["line"] = (csr(problems.poisson_1d_fd(8)[0]), 9, 0x038, 4)
    # 7-point: strides 5 and 6 both fit, 6 is looked at first, 5 divides the 20 rows
    out["seven_point"] = (banded(20, [-6, -5, -1, 0, 1, 5, 6], [-1.0, -2.0, -3.0, 12.0, -3.0, -2.0, -1.0]), 5, 0x1BB, 10)
    return out


@pytest.mark.parametrize("name", sorted(square_cases()))
def test_stencil(name, stencil_of):
    A, W, umask, interior = square_cases()[name]
    got_W, values, mask, pid, hot = stencil_of(A)
    assert got_W == W and np.bitwise_or.reduce(mask) == umask
    assert_rebuilds(A, pid, values, mask, window_3x3(W))
    assert mask[pid[interior]] == umask
    if stencil_of is stencil_by_twin:
        assert hot == pid[interior]


def refused_cases():
    eye = sp.identity(12, format="lil")
    ten = eye.copy()
    ten[5, 0:10] = 1.0
    return {
        "ten_entries": csr(ten),
        "25_point": banded(49, [c * 7 + d for c in range(-2, 3) for d in range(-2, 3)], [1.0] * 25),
        "no_slot": banded(31, [-7, -2, 0, 2, 7], [-1.0, -1.0, 4.0, -1.0, -1.0]),      # 2 is no slot of stride 6, 7 or 8
        "two_rows": csr(np.array([[2.0, -1.0], [-1.0, 2.0]])),                         # 1-D wants three rows
    }


@pytest.mark.parametrize("name", sorted(refused_cases()))
def test_stencil_refusals(name, stencil_of):
    assert stencil_of(refused_cases()[name]) is None


def test_shortest_line(stencil_of):
    assert stencil_of(banded(3, [-1, 0, 1], [-1.0, 2.0, -1.0]))[0] == 3


# ---- operators with live boundary rows (tests/grid_ops.py): entries across the end of a line ----------------------------
def line_end_cases():
    """name -> (A, W, union mask, crosses a line end): small versions of the operators of test_grid_shapes_gpu.py."""
    import grid_ops as G
    return {
        # x-periodic 5-point: the wrap-around links are the slots 2 and 6 of the grid's own stride
        "periodic5": (G.grid_op(7, 6, 0x0BA, "const", periodic_x=True), 7, 0x0FE, True),
        "periodic9": (G.grid_op(7, 6, 0x1FF, "const", periodic_x=True), 7, 0x1FF, True),
        # 7-point on 4 x 5: 5 is looked at first and divides the 20 rows -- the sheared stride, the other orientation
        "sheared7_4x5": (G.grid_op(4, 5, 0x1BB, "const"), 5, 0x0FE, True),
        # the mirror, 5 x 4: 6 does not divide 20, the grid's own stride does
        "plain7_5x4": (G.grid_op(5, 4, 0x1BB, "const"), 5, 0x1BB, False),
        # the other orientation never shears on a whole rectangle: its own stride is looked at first and divides
        "plain7b_7x6": (G.grid_op(7, 6, 0x0FE, "const"), 7, 0x0FE, False),
        # live boundary rows alone cross nothing
        "plain9_7x6": (G.grid_op(7, 6, 0x1FF, "const"), 7, 0x1FF, False),
        "ragged5": (G.grid_op(7, 6, 0x0BA, "const", rows=37), 7, 0x0BA, False),
    }


@pytest.mark.parametrize("name", sorted(line_end_cases()))
def test_operators_with_live_boundary_rows_are_linear(name, stencil_of):
    """The twins read an operator by linear offsets only: an x-periodic or sheared one decodes like any other and the
    decoded table IS the matrix; whether an entry then crosses a line end is a property the twin reports, not a refusal."""
    import grid_ops as G
    A, W, umask, crosses = line_end_cases()[name]
    got_W, values, mask, pid, _hot = stencil_of(A)
    assert got_W == W and np.bitwise_or.reduce(mask) == umask
    assert_rebuilds(A, pid, values, mask, window_3x3(W))
    assert (G.line_end_coupling(A, W).size > 0) == crosses
    if stencil_of is stencil_by_twin:
        S = ops.StencilTwin.from_patterns(record(A), A.shape)
        assert S.line_end_coupling is crosses
        if crosses:
            assert not S.gs_ok


def test_generated_operators_keep_their_boundary_couplings():
    import grid_ops as G
    for slots, per_row in ((0x0BA, 5), (0x1BB, 7), (0x0FE, 7), (0x1FF, 9)):
        for values in ("const", "row"):
            A = G.grid_op(9, 8, slots, values)
            assert A.has_sorted_indices and A.indices.dtype == np.int32 and A.shape == (72, 72)
            lens = np.diff(A.indptr)
            assert lens.max() == per_row and lens.min() >= 3 and lens[4 * 9 + 4] == per_row     # no identity rows
            d = A.diagonal()
            assert np.all(d > abs(A).sum(axis=1).A1 - d) and np.all(np.abs(A.data) >= 0.5)
            B = G.grid_op(9, 8, slots, values, rows=60)
            assert B.shape == (60, 60) and (B != A[:60, :60]).nnz == 0
    A = G.grid_op(9, 8, 0x0BA, "const", periodic_x=True)
    assert A[8, 0] != 0 and A[0, 8] != 0 and A[71, 63] != 0 and np.diff(A.indptr).min() == 4


def test_decoder_refusals():
    one = np.array([0, 2], np.int32)
    val = np.ones(10)
    dec = twins.decode_window(one, np.array([1, 2]), val, 4, {1: 0, 2: 3}.get)
    assert dec[0].tolist() == [1.0, 0.0, 0.0, 1.0] and dec[1].tolist() == [0x9]
    assert twins.decode_window(one, np.array([1, 2]), val, 4, {1: 0, 2: 0}.get) is None         # one slot hit twice
    assert twins.decode_window(one, np.array([1, 2]), val, 4, {1: 0}.get) is None               # 2 is no slot
    assert twins.decode_window(one, np.array([2, 1]), val, 4, {1: 0, 2: 3}.get) is None         # descending
    assert twins.decode_window(one, np.array([1, 1]), val, 4, {1: 0, 2: 3}.get) is None         # not ascending
    assert twins.decode_window(np.array([0, 10], np.int32), np.arange(10), val, 9, lambda o: min(o, 8)) is None
    assert twins.decode_window(np.array([0, 5], np.int32), np.arange(5), val, 4, slot_of=lambda o: min(o, 3)) is None


def test_pattern_limit(L):
    """More patterns than lmg_stencil_limits allows: refused by from_patterns, before it decodes anything."""
    mp = ctypes.c_int32(0)
    assert L.lmg_stencil_limits(ctypes.addressof(mp)) == 0
    limit = int(mp.value)

    def chain(k):
        """k rows, k patterns: an entry of its own value next to the diagonal in every row but the three-point row 1."""
        M = sp.lil_matrix((k, k))
        for i in range(k):
            M[i, i + 1 if i + 1 < k else i - 1] = i + 3.0
        M[1, 0:3] = (-1.0, 2.0, -1.0)
        return csr(M)

    S = ops.StencilTwin.from_patterns(record(chain(limit)), (limit, limit))
    assert S is not None and (S.npat, S.W, S.umask, S.hot) == (limit, limit, 0x038, 1)
    assert ops.StencilTwin.from_patterns(record(chain(limit + 1)), (limit + 1, limit + 1)) is None
    assert stencil_by_functions(chain(limit + 1)) is not None


def test_hot_pattern_ties():
    counts = np.array([7, 3, 3, 5, 9])
    assert twins.hot_pattern([], None) == -1
    assert twins.hot_pattern([3], None) == 3                      # one candidate: the counts are not looked at
    assert twins.hot_pattern([1, 2], counts) == 1                 # equal counts: the lower id
    assert twins.hot_pattern([1, 2, 3], counts) == 3              # else the larger count


# ---- transfers ------------------------------------------------------------------------------------------------------------
def parity_counts(pid, W, npat):
    """counts[line parity][column parity][id] of the rows of a grid with line stride W."""
    rows = np.arange(pid.size)
    key = ((rows // W) % 2 * 2 + rows % W % 2) * npat + pid
    return np.bincount(key, minlength=4 * npat).reshape(2, 2, npat)


@pytest.mark.parametrize("s", [5, 9])
def test_prolongation(s):
    P = csr(problems.tensor_interpolator_2d(s))
    W, Wc = s, (s + 1) // 2
    gm = (W, Wc, 1, 1, 0)
    assert gm in ops.RowPatterns.grid_map_candidates(P.shape)
    pid, ptr, off, val = pattern_table(P, gm)
    p_val, p_mask = twins.decode_window(ptr, off, val, 4, twins.slot_2x2(Wc))
    assert_rebuilds(P, pid, p_val, p_mask, [0, 1, Wc, Wc + 1], gm)
    # rows (0, 0), (0, 1), (1, 0), (1, 1) of the fine grid: coincident node, between two nodes of a line, between two lines,
    # in the middle of a cell
    ee, eo, oe, oo = (int(pid[r]) for r in (0, 1, W, W + 1))
    assert [p_mask[p] for p in (ee, eo, oe, oo)] == [0x1, 0x3, 0x5, 0xF]
    pairs, pval = twins.prolong_hot_pairs(p_val, p_mask, parity_counts(pid, W, len(p_mask)))
    assert pairs == [ee | eo << 8, oe | oo << 8]
    assert pval == [1.0, 0.5, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25, 0.25]


def test_prolongation_hot_pairs_follow_the_counts():
    """Two patterns with the slots of a parity class: the more frequent one there, the first of equally frequent ones; a
    class without a pattern of its slots leaves its line parity without a pair, and zeros in the values."""
    p_mask = np.array([0x1, 0x3, 0x1, 0x3, 0x5, 0xF], np.int32)
    p_val = np.arange(24.0)
    counts = np.zeros((2, 2, 6), np.int64)
    counts[0, 0, [0, 2]] = 4, 6
    counts[0, 1, [1, 3]] = 5, 5
    counts[1, 1, 5] = 2
    counts[1, 1, 1] = 9                                            # frequent, but not the slots of that class
    pairs, pval = twins.prolong_hot_pairs(p_val, p_mask, counts)
    assert pairs == [2 | 1 << 8, -1]
    assert pval == [8.0, 4.0, 5.0, 0.0, 0.0, 20.0, 21.0, 22.0, 23.0]


def test_prolongation_refusals():
    P = problems.tensor_interpolator_2d(5).tolil()
    gm = (5, 3, 1, 1, 0)
    P[2 * 5 + 2, 1 * 3 + 1 + 3] = 0.125                            # fine row (2, 2), an even line, reaches coarse line 2
    pid, ptr, off, val = pattern_table(csr(P), gm)
    p_val, p_mask = twins.decode_window(ptr, off, val, 4, twins.slot_2x2(3))
    assert p_mask[pid[12]] == 0x5
    assert twins.prolong_hot_pairs(p_val, p_mask, parity_counts(pid, 5, len(p_mask))) is None
    P = problems.tensor_interpolator_2d(5).tolil()
    P[2 * 5 + 2, 1 * 3 + 1 + 2] = 0.125                            # offset 2 is outside the 2 x 2 window
    pid, ptr, off, val = pattern_table(csr(P), gm)
    assert twins.decode_window(ptr, off, val, 4, twins.slot_2x2(3)) is None


def restrict_by_functions(Rm, W, gm):
    pid, ptr, off, val = pattern_table(Rm, gm)
    r_val, r_mask = twins.decode_window(ptr, off, val, 9, twins.slot_3x3(W))
    full = [p for p in range(len(r_mask)) if r_mask[p] == 0x1FF]
    return r_val, r_mask, pid, twins.hot_pattern(full, np.bincount(pid))


def restrict_by_twin(Rm, W, gm):
    R = record(Rm, gm)
    T = ops.RestrictTwin.from_patterns(R, Rm.shape)
    assert T.pid is R.pid and (T.nc, T.Wc, T.n, T.W, T.npat) == (Rm.shape[0], gm[0], Rm.shape[1], W, R.npat)
    assert T.r_val.dtype == torch.float64 and T.r_mask.dtype == torch.int32
    assert list(T._hot_val) == list(T.r_val.numpy()[T.hot * 9: T.hot * 9 + 9])
    return T.r_val.numpy(), T.r_mask.numpy(), R.pid.numpy(), T.hot


@pytest.mark.parametrize("via", [restrict_by_functions, restrict_by_twin])
@pytest.mark.parametrize("s", [5, 9])
def test_restriction(s, via):
    Rm = csr(problems.tensor_interpolator_2d(s).T)
    W, Wc = s, (s + 1) // 2
    gm = (Wc, 2 * W, 0, 0, 1)
    assert gm in ops.RowPatterns.grid_map_candidates(Rm.shape)
    r_val, r_mask, pid, hot = via(Rm, W, gm)
    assert_rebuilds(Rm, pid, r_val, r_mask, window_3x3(W), gm)
    # the hot pattern: the one with all nine slots that most rows have -- the coarse nodes off the boundary
    counts = np.bincount(pid)
    full = [p for p in range(len(r_mask)) if r_mask[p] == 0x1FF]
    assert hot in full and counts[hot] == max(counts[p] for p in full) and hot == pid[Wc + 1]


def test_builder_overrides_refuse_what_the_formats_do_not_have():
    """tile_rows / colmode of PackedCSR.from_csr and colmode of SellCSR.from_csr are checked before anything is built."""
    A = SimpleNamespace(shape=(4, 4), nnz=4, vals=torch.zeros(4, dtype=torch.float64))
    for bad in (0, 256, 1024):
        with pytest.raises(ValueError):
            ops.PackedCSR.from_csr(A, tile_rows=bad)
    for bad in (-1, 2):
        with pytest.raises(ValueError):
            ops.PackedCSR.from_csr(A, colmode=bad)
    # (a host matrix gets no sliced-ELL twin at all, whatever is asked for)
    assert ops.SellCSR.from_csr(A, colmode=2) is None
