"""The 2-D learned transfer operators on the device: the stages of NeuralMG_2D.define_hierarchy
(learn_multigrid/solvers/Multigrid.py:373-765) around the caller's `model.predict`, driven from here and executed by
csrc/nmg2d.hip (the rules they follow: DESIGN.md section 3).  The network is the caller's object: anything with
`.predict(array (p, 43)) -> array (p, 31)`.

Per level:  [cut]  ->  domain check  ->  C/F split (host, lmg_host_greedy_cf)  ->  patches  ->  (patches - mean) / std on
the host with NumPy, so that the model is shown the reference's bits  ->  model.predict  ->  fold into B  ->  Q = B / row sums
->  M_c = (Q^T M) Q by the device SpGEMM.  Everything between the split and the product works on one ops.DeviceCSR of M
with sorted rows; no n x n or n x n_c array exists.  Across the bus go: M's arrays for the split of a level after the first,
the coarse ranks, the patches (down), the predictions (up), one status word per stage and a few sizes.

A matrix the rules cannot take is refused with a Refused (a ValueError) that names the rule and the first node it fails at --
where the reference crashes late (`scaling_vnodes` answers a string), overruns the slots of its own patch, or pairs values
with the wrong columns."""
import numpy as np
import scipy.sparse as sp
import torch

from . import ops

I32, I64, F64 = torch.int32, torch.int64, torch.float64

RULE_TEXT = {
    "negative_offdiagonal": "the mass matrix has a negative off-diagonal entry",
    "diagonal": "the mass matrix has no positive diagonal entry",
    "valence": "a coarse node has 8 or more positive neighbours (the patches hold 6, two patches 7)",
    "few_neighbours": "a coarse node has fewer than 2 neighbours",
    "isolated_neighbour": "a neighbour of a coarse node has no positive neighbour but that node",
    "second_neighbours": "a coarse node has more than 6 coarse second neighbours",
    "index_range": "an index is outside the matrix, or a fill index names a node that is not coarse",
}


class Refused(ValueError):
    """A rule of the 2-D learned transfers does not hold: .rule (a key of RULE_TEXT) at .node."""

    def __init__(self, rule, node):
        super().__init__("NeuralMG_2D: %s: node %d (rule %r)" % (RULE_TEXT.get(rule, rule), node, rule))
        self.rule, self.node = rule, int(node)


def canonical(M):
    """M as float64 SciPy CSR with sorted rows, duplicates summed and explicit zeros dropped; square or ValueError."""
    M = sp.csr_matrix(M, dtype=np.float64)
    if M.shape[0] != M.shape[1]:
        raise ValueError("NeuralMG_2D: the mass matrix must be square, got %s" % (M.shape,))
    if not M.has_canonical_format or np.any(M.data == 0.0):
        M = M.copy()
        M.sum_duplicates()
        M.eliminate_zeros()
    return M


def _refusal(status, node_of):
    hit = ops.nmg2d_read_status(status)
    if hit is not None:
        raise Refused(hit[0], node_of(hit[1]))


def check_domain(dM):
    """Refuses a DeviceCSR outside the domain of the rules (whole matrix, one read back)."""
    status = ops.nmg2d_status(dM.device)
    ops.nmg2d_check(dM, status)
    _refusal(status, lambda row: row)


def cf_split(M):
    """(CC, rank) of the SciPy CSR matrix M: the coarse nodes ascending (int64) and every node's position among them
    (int32, -1 for a fine node)."""
    is_coarse = ops.host_greedy_cf(M)
    CC = np.flatnonzero(is_coarse)
    rank = np.where(is_coarse > 0, np.cumsum(is_coarse, dtype=np.int64) - 1, -1).astype(np.int32)
    return CC, rank


def rank_of(CC, n):
    """rank (int32, n) of a given list of coarse nodes; ValueError unless they ascend inside [0, n)."""
    CC = np.asarray(CC, dtype=np.int64).reshape(-1)
    if CC.size and (CC[0] < 0 or CC[-1] >= n or np.any(np.diff(CC) <= 0)):
        raise ValueError("NeuralMG_2D: the coarse nodes must ascend inside [0, %d)" % n)
    rank = np.full(n, -1, dtype=np.int32)
    rank[CC] = np.arange(CC.size, dtype=np.int32)
    return rank


class Patches:
    """What extract_patches leaves on the device: patches (p, 43) float64, fill_idx (p, 31) int32, the coarse node of every
    patch and, per coarse node, its last patch.  The first patch of coarse node r is patch r; the second patches of the
    nodes with 7 neighbours follow all first ones in coarse order."""
    __slots__ = ("patches", "fill_idx", "node", "last")

    def __init__(self, patches, fill_idx, node, last):
        self.patches, self.fill_idx, self.node, self.last = patches, fill_idx, node, last


def extract_patches(dM, CC, rank):
    """CC, rank: int32 device tensors (coarse nodes ascending; position among them or -1).  dM must have passed
    check_domain."""
    dev, nc = dM.device, CC.numel()
    status = ops.nmg2d_status(dev)
    extra = torch.empty(nc, dtype=I32, device=dev)
    ops.nmg2d_count(dM, CC, extra, status)
    _refusal(status, lambda r: int(CC[r]))
    # placement: patch r is the first of coarse node r, the second ones follow in coarse order
    twice = torch.nonzero(extra).flatten()
    node = torch.cat([CC, CC[twice]]).contiguous()
    variant = torch.cat([torch.zeros(nc, dtype=I32, device=dev), torch.ones(twice.numel(), dtype=I32, device=dev)])
    last = torch.arange(nc, dtype=I32, device=dev)
    last[twice] = nc + torch.arange(twice.numel(), dtype=I32, device=dev)
    p = node.numel()
    patches = torch.empty((p, 43), dtype=F64, device=dev)
    fill_idx = torch.empty((p, 31), dtype=I32, device=dev)
    ops.nmg2d_patches(dM, node, variant, rank, patches, fill_idx, status)
    _refusal(status, lambda j: int(node[j]))
    return Patches(patches, fill_idx, node, last)


def fill_B(res, fill_idx, last, rank, nc):
    """(B, d_neighs): the DeviceCSR (n, nc) the predictions res (p, 31) fold into, columns ascending, and the (nc, 6) int32
    array of every coarse node's coarse second neighbours, padded with -1.  fill_idx (p, 31), last (nc) and rank (n): int32
    device tensors."""
    dev, n, p = res.device, rank.numel(), fill_idx.shape[0]
    if tuple(res.shape) != (p, 31):
        raise ValueError("NeuralMG_2D: the model returned %s for %d patches, expected (%d, 31)" % (tuple(res.shape), p, p))
    status = ops.nmg2d_status(dev)
    keys = torch.empty(p * 31, dtype=I64, device=dev)
    ops.nmg2d_contrib(nc, fill_idx, rank, keys, status)
    _refusal(status, lambda j: int(fill_idx[j, 0]))
    # stable: inside a run of equal keys the slots stay in patch order, the order the fold depends on
    keys, slot = torch.sort(keys, stable=True)
    valid = int((keys != torch.iinfo(I64).max).sum())
    first = torch.ones(valid, dtype=torch.bool, device=dev)
    first[1:] = keys[1:valid] != keys[:valid - 1]
    start = torch.cat([torch.nonzero(first).flatten(), torch.tensor([valid], dtype=I64, device=dev)])
    ne = start.numel() - 1
    row, col = torch.empty(ne, dtype=I32, device=dev), torch.empty(ne, dtype=I32, device=dev)
    val = torch.empty(ne, dtype=F64, device=dev)
    ops.nmg2d_fold(start, keys, slot, res.reshape(-1), nc, row, col, val)
    rowptr = torch.zeros(n + 1, dtype=I32, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(row.long(), minlength=n), 0).to(I32)
    d_neighs = torch.empty((nc, 6), dtype=I32, device=dev)
    ops.nmg2d_dneighs(last, fill_idx, rank, d_neighs)
    return ops.DeviceCSR(rowptr, col, val, (n, nc)), d_neighs


def coarse_mass(dQ, dM):
    """M_c = (Q^T M) Q, evaluated left to right like SciPy evaluates `Q.T @ mass @ Q` (:763): the same bits."""
    return ops.spgemm(ops.spgemm(dQ.transpose(), dM), dQ)


def define_hierarchy(model, M, mean, std, levels, device, timings=None):
    """[Q_0, ..., Q_{levels-2}] as SciPy CSR matrices with unit row sums (Multigrid.py:741-765).  timings: a dict that
    receives the seconds per stage, summed over the levels (each stage is synchronised for it)."""
    import time

    def lap(name, t0):
        if timings is not None:
            torch.cuda.synchronize(device)
            timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    out = []
    host = canonical(M)
    dM = ops.DeviceCSR.from_scipy(host, device)
    for lev in range(levels - 1):
        t = time.perf_counter()
        if lev:
            dM = ops.nmg2d_cut(dM, d_neighs)
            host = dM.to_scipy()
            t = lap("cut", t)
        check_domain(dM)
        t = lap("check", t)
        CC, rank = cf_split(host)
        dCC = torch.from_numpy(CC.astype(np.int32)).to(device)
        drank = torch.from_numpy(rank).to(device)
        t = lap("split", t)
        P = extract_patches(dM, dCC, drank)
        patches = P.patches.cpu().numpy()
        t = lap("patches", t)
        data = (patches - mean) / std                                            # :755, on the host like the reference
        res = np.ascontiguousarray(np.asarray(model.predict(data), dtype=np.float64))
        t = lap("model", t)
        dB, d_neighs = fill_B(torch.from_numpy(res).to(device), P.fill_idx, P.last, drank, CC.size)
        dQ = ops.nmg2d_normalize(dB)
        t = lap("fill", t)
        out.append(dQ.to_scipy())
        if lev < levels - 2:                      # (the reference also forms the product nobody reads, after the last Q)
            dM = coarse_mass(dQ, dM)
            t = lap("product", t)
    return out
