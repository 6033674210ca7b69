"""NumPy statement of what learnmultigrid_amd/mesh.py computes on the device -- structured construction, refinement,
boundary nodes, identity rows -- and the meshes the CPU and GPU tests share.  Written for this project from the rules of
DESIGN.md section 3 ("Meshes"); the tests compare the device with it bit for bit.

A slot s = 3 e + k is the directed edge conn[e][k] -> conn[e][(k + 1) % 3].  Slots with the same unordered end nodes are
one edge; its head is the smallest of them.  Midpoints are numbered n, n + 1, ... in the order of the head slots."""
import numpy as np
import scipy.sparse as sp


def construct(h_el, v_el):
    """(p, conn) of h_el x v_el squares on the unit square: nodes row-major, h fastest; square k gives (k, k+1, k+W+1) and
    then (k, k+W+1, k+W)."""
    W = h_el + 1
    x, y = np.linspace(0, 1, h_el + 1), np.linspace(0, 1, v_el + 1)
    p = np.stack([np.tile(x, v_el + 1), np.repeat(y, h_el + 1)], axis=1)
    k = (np.arange(v_el)[:, None] * W + np.arange(h_el)[None, :]).ravel()
    conn = np.stack([k, k + 1, k + W + 1, k, k + W + 1, k + W], axis=1).reshape(-1, 3)
    return p, conn.astype(np.int64)


def edges(conn):
    """Per slot: (left, right, head slot, length of its run)."""
    conn = np.asarray(conn, dtype=np.int64)
    left, right = conn.ravel(), np.roll(conn, -1, axis=1).ravel()
    key = (np.minimum(left, right) << 32) | np.maximum(left, right)
    _, first, inverse, counts = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    return left, right, first[inverse], counts[inverse]          # (return_index gives the first = smallest slot)


def n_edges(conn):
    _l, _r, head, _c = edges(conn)
    return int(np.unique(head).size)


def refine(p, conn, ratios=None):
    """One refinement.  ratios[j] belongs to new node n + j (None: midpoints)."""
    p, conn = np.asarray(p, dtype=np.float64), np.asarray(conn, dtype=np.int64)
    n, ne = p.shape[0], conn.shape[0]
    left, right, head, _c = edges(conn)
    heads = np.unique(head)                                      # ascending
    mid = n + np.searchsorted(heads, head)                       # per slot: the node on its edge
    r = np.full(heads.size, 0.5) if ratios is None else np.asarray(ratios, dtype=np.float64)
    assert r.shape == (heads.size,)
    new = r[:, None] * p[left[heads]] + (1 - r)[:, None] * p[right[heads]]
    t = mid.reshape(ne, 3)
    kids = np.stack([t[:, 0], conn[:, 1], t[:, 1],
                     t[:, 1], conn[:, 2], t[:, 2],
                     t[:, 0], t[:, 1], t[:, 2],
                     conn[:, 0], t[:, 0], t[:, 2]], axis=1).reshape(4 * ne, 3)
    return np.vstack([p, new]), kids


def irregular_ratios(n_new, seed):
    """The ratios of refine(False, seed=seed): the reference draws a + (b - a) * rand() once per new edge, in the order
    it numbers them, a = 0.3, b = 0.7."""
    return 0.3 + (0.7 - 0.3) * np.random.RandomState(seed).rand(n_new)


def boundary(n, conn):
    """bool (n,): node i is an end of an edge that occurs in one slot only."""
    left, right, _h, count = edges(conn)
    mask = np.zeros(n, dtype=bool)
    mask[left[count == 1]] = True
    mask[right[count == 1]] = True
    return mask


def identity_rows(A, rhs, mask, value=None):
    """(A', rhs'): masked rows of the CSR A get 1 on the diagonal and 0 on their other stored entries (kept stored),
    rhs 0 or value there."""
    A = sp.csr_matrix(A, copy=True)
    rhs = np.array(rhs, dtype=np.float64).ravel()
    for i in np.flatnonzero(mask):
        sl = slice(A.indptr[i], A.indptr[i + 1])
        assert i in A.indices[sl]
        A.data[sl] = (A.indices[sl] == i).astype(np.float64)
        rhs[i] = 0.0 if value is None else value[i]
    return A, rhs


def areas(p, conn):
    a, b, c = p[conn[:, 0]], p[conn[:, 1]], p[conn[:, 2]]
    return 0.5 * np.abs((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (c[:, 0] - a[:, 0]) * (b[:, 1] - a[:, 1]))


def unit_square_boundary(p):
    return (p[:, 0] == 0) | (p[:, 0] == 1) | (p[:, 1] == 0) | (p[:, 1] == 1)


# ---- the meshes of the tests ---------------------------------------------------------------------------------------------
def balanced(ne):
    from learnmultigrid_amd.mesh import find_balanced_couple
    return find_balanced_couple(ne)


def jittered_flipped():
    """problems.jittered_mesh_2d(17) with every third element's orientation flipped."""
    from learnmultigrid_amd import problems as P
    p, conn = P.jittered_mesh_2d(17)
    conn = np.array(conn, dtype=np.int64)
    conn[::3] = conn[::3][:, [0, 2, 1]]
    return p, conn


def three_on_one_edge():
    """Three triangles that share the edge 0 - 1: a run of length 3."""
    p = np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 1.0], [0.5, -1.0], [0.25, 0.5]])
    return p, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int64)


def with_unused_nodes():
    """Mesh2D(6) with two nodes no element refers to, one between the used ones and one at the end."""
    p, conn = construct(*balanced(6))
    at = 5
    p = np.vstack([p[:at], [[7.0, 7.0]], p[at:], [[9.0, 9.0]]])
    conn = np.where(conn >= at, conn + 1, conn)
    return p, conn


def l_shape():
    """Mesh2D(16) without the elements of the quadrant x > 1/2, y > 1/2 (their nodes stay, some unused)."""
    p, conn = construct(4, 4)
    c = p[conn].mean(axis=1)
    keep = ~((c[:, 0] > 0.5) & (c[:, 1] > 0.5))
    return p, conn[keep]


def fan(m):
    """A closed fan of m triangles round node 0: its row has m + 1 columns."""
    ang = 2 * np.pi * np.arange(m) / m
    p = np.vstack([[[0.0, 0.0]], np.stack([np.cos(ang), np.sin(ang)], axis=1)])
    ring = 1 + np.arange(m)
    conn = np.stack([np.zeros(m, dtype=np.int64), ring, 1 + (np.arange(m) + 1) % m], axis=1)
    return p, conn


CASES = {
    "one": lambda: construct(*balanced(1)),
    "5x3": lambda: construct(*balanced(15)),
    "25": lambda: construct(*balanced(25)),
    "64x64": lambda: construct(*balanced(64 * 64)),
    "jitter_flipped": jittered_flipped,
    "run3": three_on_one_edge,
    "unused": with_unused_nodes,
}
