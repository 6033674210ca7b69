"""What the NeuralMG_2D tests share (test-only): the g8_nmg2d_* fixtures unpacked per level, the model that replays their
stored predictions, the matrices every refusal is crafted on, and P1 mass matrices of structured triangulations."""
import numpy as np
import scipy.sparse as sp

from conftest import coo_from, load_golden

CASES = ("k4", "k16", "k16_jitter", "k16_valence7", "k16_random")
EPS = np.finfo(np.float64).eps


def load_case(name):
    """(g, levels): the fixture and, per level, a dict M, CC, patches, fill_idxs, res, B, Q, d_neighs, Mc, Mcut, all as the
    reference produced them (CSR for the matrices).  Q lies on B's pattern; the M of a later level is the Mcut before it."""
    g = load_golden("g8_nmg2d_" + name)
    out = []
    for lev in range(int(g["levels"]) - 1):
        pre = "l%d_" % lev
        B = coo_from(g, pre + "B")
        B.sort_indices()
        Mc = coo_from(g, pre + "Mc").tocoo()
        keep = g[pre + "Mcut_keep"]
        out.append(dict(M=coo_from(g, "l0_M") if lev == 0 else out[-1]["Mcut"], CC=g[pre + "CC"].astype(np.int64),
                        patches=g[pre + "patches"], fill_idxs=g[pre + "fill_idxs"].astype(np.int64),
                        res=g[pre + "res"].astype(np.float64), B=B, Q=sp.csr_matrix((g[pre + "Q_data"], B.indices, B.indptr), B.shape),
                        d_neighs=g[pre + "d_neighs"].astype(np.int64), Mc=Mc.tocsr(),
                        Mcut=sp.csr_matrix((Mc.data[keep], (Mc.row[keep], Mc.col[keep])), shape=Mc.shape)))
    return g, out


def q_bound(B):
    """|Q - Q_ref| <= 2 k eps |Q_ref|, k the longest row of B: both row sums carry at most (k - 1) eps relative error
    (k positive terms, any order), each division eps / 2."""
    return 2 * int(np.diff(sp.csr_matrix(B).indptr).max()) * EPS


def product_bound(Q, M):
    """Two evaluations of (Q^T M) Q from the same Q and M differ by at most 2 (m - 1) eps of an entry: Q^T M comes out
    the same (each of its entries is one sum in one order), but an entry of the second product is a sum of m positive terms,
    m at most the longest row of Q^T M, taken in the order in which the rows of Q^T M are STORED -- SciPy leaves them in
    the order of its hash list, the device SpGEMM in ascending columns -- and each order carries (m - 1) eps."""
    T = sp.csr_matrix(sp.csr_matrix(Q).T) @ sp.csr_matrix(M)
    return 2 * (int(np.diff(T.indptr).max()) - 1) * EPS


def same_pattern(X, Y):
    X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
    return X.shape == Y.shape and np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)


class StoredModel:
    """predict() number l returns the stored res of level l.  At level 0 it insists on being shown (patches - mean) / std of
    the stored patches bit for bit; at later levels, whose patches inherit the rounding of Q_0, within `rtol`."""

    def __init__(self, g, levels, rtol=0.0):
        self.g, self.levels, self.rtol, self.calls = g, levels, rtol, 0
        self.shown = []

    def predict(self, data):
        lev = self.levels[self.calls]
        want = (lev["patches"] - self.g["mean"]) / self.g["std"]
        self.shown.append(np.array(data))
        if self.calls == 0:
            assert np.array_equal(data, want)
        else:
            # (a relative change of the patch values, seen through the subtraction and the division)
            room = self.rtol * (np.abs(lev["patches"]) + np.abs(self.g["mean"])) / np.abs(self.g["std"])
            assert data.shape == want.shape and np.all(np.abs(data - want) <= room)
        self.calls += 1
        return lev["res"].copy()


class FormulaModel:
    """An element-wise model: positive predictions from the first 31 features; every call is kept."""

    def __init__(self):
        self.calls = []

    def predict(self, data):
        out = 0.25 + 0.125 * np.abs(np.sin(1e3 * data[:, :31] + np.arange(31.0)))
        self.calls.append((np.array(data), out))
        return out


def graph_matrix(n, edges, diag=1.0, off=0.1):
    M = sp.lil_matrix((n, n))
    M.setdiag(diag)
    for e, (a, b) in enumerate(edges):
        M[a, b] = M[b, a] = off * (1.0 + 0.01 * e)
    return M.tocsr()


def refusal_cases():
    """{name: (M, rule, node)}: each on at most 30 nodes, the rule it breaks and the first node it breaks it at."""
    k4 = coo_from(load_golden("g4_structured2d_k4"), "M")
    neg = k4.tolil()
    neg[3, 4] = -abs(neg[3, 4]) - 1e-3
    nodiag = k4.tolil()
    nodiag[5, 5] = 0.0
    ring = [(j, j % 8 + 1) for j in range(1, 9)]
    return {
        "negative off-diagonal": (neg.tocsr(), "negative_offdiagonal", 3),
        "zero diagonal": (nodiag.tocsr(), "diagonal", 5),
        "8 neighbours": (graph_matrix(9, [(0, j) for j in range(1, 9)] + ring), "valence", 0),
        "one neighbour": (graph_matrix(6, [(j, j + 1) for j in range(5)]), "few_neighbours", 0),
        "neighbour with no other neighbour": (graph_matrix(6, [(0, 1), (0, 2), (2, 3), (3, 4), (4, 5)]), "isolated_neighbour", 0),
        "7 coarse second neighbours": (graph_matrix(12, [(0, 1), (0, 2), (0, 3), (0, 4), (1, 5), (1, 6), (2, 7), (2, 8), (3, 9),
                                                         (3, 10), (4, 11)]), "second_neighbours", 0),
    }


def p1_mass(nx, ny, seed=None):
    """P1 mass matrix of the nx x ny structured triangulation of the unit square (cells cut along one diagonal), rows in
    grid order; seed: every entry replaced by a random positive value on the same pattern (not symmetric)."""
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (j * nx + i).ravel()
    tris = np.concatenate([np.stack([a, a + 1, a + nx + 1], 1), np.stack([a, a + nx + 1, a + nx], 1)])
    loc = hx * hy / 24.0 * (np.ones((3, 3)) + np.eye(3))
    rows, cols = np.repeat(tris, 3, axis=1).ravel(), np.tile(tris, (1, 3)).ravel()
    M = sp.coo_matrix((np.tile(loc.ravel(), len(tris)), (rows, cols)), shape=(nx * ny, nx * ny)).tocsr()
    if seed is not None:
        M.data = 0.5 + np.random.RandomState(seed).random_sample(M.nnz)
    return M
