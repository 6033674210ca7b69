"""Grid operators with LIVE boundary rows for the tests (no kernel reads this file): every node of a Wg x Hg grid couples
to all of its in-grid neighbours, boundary nodes included -- natural boundary conditions, eliminated Dirichlet nodes, the
local blocks cut out of a level -- where the generators of learnmultigrid_amd.problems put identity rows.  Such a matrix
is what the storage twins call it: entries at  column - row = c * W + d,  c, d in {-1, 0, 1},  and nothing else; which W
reads it that way, and whether an entry then crosses the end of a line, is the twins' business."""
import numpy as np
import scipy.sparse as sp

MASKS = (0x0BA, 0x1BB, 0x0FE, 0x1FF)          # 5-point, the two 7-point orientations, 9-point (slot s = 3 (c + 1) + d + 1)


def grid_op(Wg, Hg, slots, values, periodic_x=False, rows=None, seed=0):
    """Sorted CSR (int32 indices) of an operator on the lexicographic Wg x Hg grid, row = y * Wg + x.

    slots       one of MASKS, read for line stride Wg: node (y, x) couples to (y + c, x + d) for every slot of the mask
                whose neighbour is inside the grid.  No identity rows.
    values      "const": one off-diagonal value per slot (another set on the boundary nodes) and one diagonal -- a handful of
                distinct rows, the operator takes the row-pattern / stencil twin;
                "row": every entry distinct -- the operator takes the DIA twin.
                Off-diagonal entries are +-[0.5, 2), the diagonal is 1.5 x the absolute sum of the full stencil ("const")
                or 1.25 .. 1.75 x the row's own ("row"): strictly dominant, Jacobi contracts, and a dropped entry moves
                the result by O(1), not by rounding.
    periodic_x  the links to (y, x - 1) and (y, x + 1) wrap around the line: column Wg - 1 couples to column 0 of the SAME
                line and back (offsets -(Wg - 1) and Wg - 1: slots 2 and 6 of stride Wg).  Diagonal links do not wrap.
    rows        n': the leading principal n' x n' block (n' % Wg != 0: a ragged last line)."""
    assert slots in MASKS and values in ("const", "row") and Wg >= 3 and Hg >= 2
    n = Wg * Hg
    rng = np.random.default_rng(seed)
    idx = np.arange(n, dtype=np.int64)
    y, x = idx // Wg, idx % Wg
    boundary = ((x == 0) | (x == Wg - 1) | (y == 0) | (y == Hg - 1)).astype(np.int64)
    table = rng.uniform(0.5, 2.0, (2, 9)) * rng.choice([-1.0, 1.0], (2, 9))      # "const": [interior / boundary][slot]
    R, C, V = [], [], []
    for s in range(9):
        if s == 4 or not (slots >> s) & 1:
            continue
        c, d = s // 3 - 1, s % 3 - 1
        yy, xx = y + c, x + d
        if periodic_x and c == 0:
            xx = xx % Wg
        ok = (yy >= 0) & (yy < Hg) & (xx >= 0) & (xx < Wg)
        r = idx[ok]
        R.append(r)
        C.append(yy[ok] * Wg + xx[ok])
        if values == "const":
            V.append(table[boundary[r], s])
        else:
            V.append(rng.uniform(0.5, 2.0, r.size) * rng.choice([-1.0, 1.0], r.size))
    R, C, V = np.concatenate(R), np.concatenate(C), np.concatenate(V)
    if values == "const":
        diag = np.full(n, 1.5 * np.abs(table[:, [s for s in range(9) if s != 4 and (slots >> s) & 1]]).sum(axis=1).max())
    else:
        diag = np.bincount(R, weights=np.abs(V), minlength=n) * rng.uniform(1.25, 1.75, n)
    A = sp.csr_matrix((np.concatenate([V, diag]), (np.concatenate([R, idx]), np.concatenate([C, idx]))), shape=(n, n))
    if rows is not None:
        assert 0 < rows <= n
        A = A[:rows, :rows].tocsr()
    A.sum_duplicates()
    A.sort_indices()
    A = sp.csr_matrix((A.data.astype(np.float64), A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)
    if values == "row":
        assert np.unique(A.data).size == A.nnz
    return A


def line_end_coupling(A, W):
    """Rows of A with an entry that the 3x3 window of stride W places across the end of a line: in column 0 a slot with
    d = -1, in column W - 1 a slot with d = +1 (what StencilTwin.gs_ok looks for, here from the matrix itself)."""
    coo = A.tocoo()
    off = coo.col.astype(np.int64) - coo.row
    d = np.full(off.shape, 9, dtype=np.int64)
    for c in (-1, 0, 1):
        dd = off - c * W
        d = np.where((np.abs(dd) <= 1) & (d == 9), dd, d)
    assert (d != 9).all(), "an entry is no slot of stride %d" % W
    col = coo.row % W
    return np.unique(coo.row[((col == 0) & (d == -1)) | ((col == W - 1) & (d == 1))])
