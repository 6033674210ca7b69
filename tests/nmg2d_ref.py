"""TEST-ONLY plain-Python restatement of the rules NeuralMG_2D's hierarchy follows ("2-D learned
transfers"): domain check, C/F split, patches and fill indices, the fold into B, Q, d_neighs and the cut.  Written from
the rules, node by node and list by list, with no care for speed: what learned_q2d.py and csrc/nmg2d.hip are compared with
where no fixture of the reference's own run exists.  Nothing in learnmultigrid_amd imports this file.

Every refusal is a Refused (a ValueError) carrying .rule and .node, in the order in which the stages meet them: rows in
ascending order for the domain, coarse nodes in ascending order for the valence, patches in patch order for the rest."""
import numpy as np
import scipy.sparse as sp

UP = {2: 6.0, 3: 3.0, 4: 2.0, 5: 1.5}
DOWN = {2: 1.0, 3: 2.0, 4: 3.0, 5: 4.0}


class Refused(ValueError):
    def __init__(self, rule, node):
        super().__init__("%s at node %d" % (rule, node))
        self.rule, self.node = rule, int(node)


def canonical(M):
    M = sp.csr_matrix(M, dtype=np.float64).copy()
    M.sum_duplicates()
    M.eliminate_zeros()
    M.sort_indices()
    return M


def row_of(M, i):
    s, e = M.indptr[i], M.indptr[i + 1]
    return [int(j) for j in M.indices[s:e]], [float(v) for v in M.data[s:e]]


def check_domain(M):
    M = canonical(M)
    if M.shape[0] != M.shape[1]:
        raise ValueError("the mass matrix must be square")
    for i in range(M.shape[0]):
        cols, vals = row_of(M, i)
        for j, v in zip(cols, vals):
            if j != i and v < 0:
                raise Refused("negative_offdiagonal", i)
        if i not in cols or vals[cols.index(i)] <= 0:
            raise Refused("diagonal", i)
    return M


def cf_split(M):
    """is_coarse (bool, n): node i is coarse iff no coarse c < i has M[c, i] > 0."""
    M = canonical(M)
    n = M.shape[0]
    barred = np.zeros(n, dtype=bool)
    coarse = np.zeros(n, dtype=bool)
    for i in range(n):
        if barred[i]:
            continue
        coarse[i] = True
        cols, vals = row_of(M, i)
        for j, v in zip(cols, vals):
            if j != i and v > 0:
                barred[j] = True
    return coarse


def drop_first_smallest(vals, *others):
    k = vals.index(min(vals))
    for lst in (vals,) + others:
        del lst[k]


def one_patch(M, c, where, row, d, coarse):
    patch = [-1.0] * 43
    idx = [-1] * 31
    k = len(where)
    if k < 2:
        raise Refused("few_neighbours", c)
    patch[0] = d
    patch[1:1 + k] = row
    for t in range(k, 6):
        patch[1 + t] = d / DOWN[k]
    idx[0] = c
    idx[1:1 + k] = where
    second = []
    for b, nb in enumerate(where):
        cols, vals = row_of(M, nb)
        g, kept_v, kept_c = None, [], []
        for j, v in zip(cols, vals):
            if j == c:
                continue
            if coarse[j] and j not in where and j not in second:
                if len(second) == 6:
                    raise Refused("second_neighbours", c)
                second.append(j)
            if j == nb:
                g = v
            elif v > 0:
                kept_v.append(v)
                kept_c.append(j)
        while len(kept_v) > 5:
            drop_first_smallest(kept_v, kept_c)
        q = len(kept_v)
        if q == 0:
            raise Refused("isolated_neighbour", c)
        block = [g] + kept_v + [g / DOWN[q + 1]] * (5 - q) if q < 5 else [g] + kept_v
        patch[7 + 6 * b: 13 + 6 * b] = block
        # the coarse nodes two steps behind this neighbour: the last three
        cand = []
        for kk in kept_c:
            c2, v2 = row_of(M, kk)
            while len(v2) > 7:
                drop_first_smallest(v2, c2)
            for j in c2:
                if coarse[j] and j != c and j not in cand:
                    cand.append(j)
        cand = cand[-3:]
        idx[13 + 3 * b: 13 + 3 * b + len(cand)] = cand
    for b in range(k, 6):
        patch[7 + 6 * b: 13 + 6 * b] = [d * UP[k]] + [d / DOWN[k]] * 5
    idx[7:7 + len(second)] = second
    return patch, idx


def extract_patches(CC, M):
    """(patches (p, 43) float64, fill_idxs (p, 31) int64) of the coarse nodes CC (ascending) of M (in the domain)."""
    M = canonical(M)
    coarse = np.zeros(M.shape[0], dtype=bool)
    coarse[np.asarray(CC, dtype=np.int64)] = True
    nodes = []
    for c in CC:
        cols, vals = row_of(M, c)
        where = [j for j, v in zip(cols, vals) if j != c and v > 0]
        row = [v for j, v in zip(cols, vals) if j != c and v > 0]
        if len(where) >= 8:
            raise Refused("valence", c)
        nodes.append((int(c), where, row, vals[cols.index(c)]))
    first, second = [], []
    for c, where, row, d in nodes:
        if len(where) == 7:
            order = sorted(range(7), key=lambda t: (row[t], t))
            for a, out in ((0, first), (1, second)):
                keep = [t for t in range(7) if t != order[a]]
                out.append((c, [where[t] for t in keep], [row[t] for t in keep], d))
        else:
            first.append((c, where, row, d))
    done = [one_patch(M, c, where, row, d, coarse) for c, where, row, d in first + second]
    return (np.array([p for p, _ in done], dtype=np.float64).reshape(-1, 43),
            np.array([i for _, i in done], dtype=np.int64).reshape(-1, 31))


def fill_B(res, idx, n, CC):
    """(B csr n x n_c, d_neighs (n_c, 6) int64 padded with -1) from the predictions res (p, 31)."""
    rank = {int(c): r for r, c in enumerate(CC)}
    nc = len(CC)
    B = {}
    dn = -np.ones((nc, 6), dtype=np.int64)

    def fold(i, j, p):
        cur = B.get((i, j), 0.0)
        B[(i, j)] = p if cur == 0 else (cur + p) / 2

    for j in range(len(res)):
        p, w = [float(x) for x in res[j]], [int(x) for x in idx[j]]
        col = rank[w[0]]
        fold(w[0], col, p[0])
        for t in range(1, 7):
            if w[t] >= 0:
                fold(w[t], col, p[t])
        dn[col] = -1
        for t in range(7, 13):
            if w[t] >= 0:
                fold(w[0], rank[w[t]], p[t])
                dn[col, t - 7] = rank[w[t]]
        for b in range(6):
            if w[1 + b] < 0:
                continue
            for t in range(13 + 3 * b, 16 + 3 * b):
                if w[t] >= 0:
                    fold(w[1 + b], rank[w[t]], p[t])
    keys = sorted(B)
    out = sp.csr_matrix((np.array([B[k] for k in keys], dtype=np.float64),
                         (np.array([k[0] for k in keys], dtype=np.int64), np.array([k[1] for k in keys], dtype=np.int64))),
                        shape=(n, nc))
    return out, dn


def normalise(B):
    """Q: every row of B divided by its sum taken in ascending column order."""
    B = sp.csr_matrix(B).copy()
    B.sort_indices()
    for i in range(B.shape[0]):
        s, e = B.indptr[i], B.indptr[i + 1]
        tot = 0.0
        for v in B.data[s:e]:
            tot = tot + float(v)
        B.data[s:e] = B.data[s:e] / tot
    return B


def cut(Mc, d_neighs):
    """Entry (i, j) of the coarse mass matrix stays iff j == i or j is in d_neighs[i]."""
    C = sp.coo_matrix(canonical(Mc))
    keep = np.array([j == i or j in d_neighs[i] for i, j in zip(C.row, C.col)], dtype=bool)
    return sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=C.shape)


def hierarchy(M, predict, mean, std, levels):
    """The per-level results of define_hierarchy(levels): a list of dicts (M, CC, patches, fill_idxs, xin, res, B, Q,
    d_neighs, Mc); the mass matrix of the next level is cut(Mc, d_neighs)."""
    out = []
    M = check_domain(M)
    for lev in range(levels - 1):
        if lev:
            M = check_domain(cut(out[-1]["Mc"], out[-1]["d_neighs"]))
        CC = np.flatnonzero(cf_split(M))
        patches, idx = extract_patches(CC, M)
        xin = (patches - mean) / std
        res = np.asarray(predict(xin), dtype=np.float64)
        B, dn = fill_B(res, idx, M.shape[0], CC)
        Q = normalise(B)
        Mc = sp.csr_matrix((sp.csr_matrix(Q.T) @ M) @ Q)
        out.append(dict(M=M, CC=CC, patches=patches, fill_idxs=idx, xin=xin, res=res, B=B, Q=Q, d_neighs=dn, Mc=Mc))
    return out
