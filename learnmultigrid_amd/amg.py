"""Classical AMG setup on the device (csrc/amg.hip): from a matrix alone to a Hierarchy.

What the reference's experiment scripts get from `pyamg.ruge_stuben_solver(A, ...)` as their algebraic baseline
(test_pyAMG.py, test_from_loading_data.py:430-433, test_virtual_extension.py:501-504), in stages that all run in parallel:

    S        = strength_device(A, theta)                     strength of connection
    split    = pmis_device(S)                                C/F split: PMIS (not Ruge-Stueben's sequential passes)
    P        = direct_interpolation_device(A, S, ...)        direct interpolation
    P        = smooth_interpolation_device(A, P, ...)        one Jacobi step on P, truncated (ops.spgemm for A P)
    H        = classical_hierarchy(A, device)                the level loop; every A_(l+1) = (P^T A) P is formed once, by
                                                             Hierarchy, and no P crosses the bus

The rules are DESIGN.md section 3, "Classical AMG setup"; tests/amg_ref.py restates them in plain Python and the kernels give
the same integers and bits.  There is no CPU path: everything but split="greedy" (the reference's own `coarsening` rule, a
host helper kept as a cross-check) is a launch on the device that holds A.
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import ops
from .ops import DeviceCSR, F64, I32

SPLITS = ("pmis", "greedy")


class Refused(ValueError):
    """A matrix the rules cannot take: .rule (ops.AMG_RULES) and .row."""

    WHY = {"candidate": "smoothed-aggregation setup refuses row %d: %s (the candidate's sum of squares over the row's "
                        "aggregate is zero or not finite)"}

    def __init__(self, rule, row):
        super().__init__(self.WHY.get(rule, "classical AMG setup refuses row %d: %s (d_i = a_ii + the couplings of its sign "
                                            "is zero or not finite)") % (row, rule))
        self.rule, self.row = rule, int(row)


def _check_unit(name, v):
    v = float(v)
    if not 0.0 <= v <= 1.0:
        raise ValueError("%s must lie in [0, 1], got %r" % (name, v))
    return v


def as_device_csr(A, device):
    """A as a DeviceCSR with sorted, duplicate-free rows on `device`: a DeviceCSR is taken as it is."""
    if isinstance(A, DeviceCSR):
        return A
    return DeviceCSR.from_scipy(sp.csr_matrix(A, dtype=np.float64), device)


def strength_device(A, theta=0.25):
    """S, the strength pattern of the DeviceCSR A as a DeviceCSR with values 1.0 (columns in A's order)."""
    if A.shape[0] != A.shape[1]:
        raise ValueError("the strength of connection needs a square matrix, got %s" % (A.shape,))
    rp, sj = ops.amg_strength(A, _check_unit("theta", theta))
    return DeviceCSR(rp, sj, torch.ones(sj.numel(), dtype=F64, device=sj.device), A.shape)


def _ranks(is_coarse, n):
    rank, n_c = ops._scan_rows(is_coarse, n)
    return rank[:n], n_c


def pmis_device(S):
    """(state, rank, n_c, rounds) of the PMIS split on the strength pattern S.  state: int32 per node (ops.AMG_COARSE,
    AMG_FINE, AMG_FINE0); rank[i]: the number of coarse nodes below i, for a coarse node its column of P.  The host reads one
    count per round -- the nodes still undecided -- so the setup cannot be captured into a graph."""
    n, dev = S.shape[0], S.device
    ST = S.transpose()
    count, state, flag, isc = (torch.empty(max(n, 1), dtype=I32, device=dev) for _ in range(4))
    ops.amg_pmis_keys(S, ST, count, state, isc)
    nb = ops.amg_pmis_blocks(n)
    left = torch.zeros(max(nb, 1), dtype=I32, device=dev)
    # the undecided nodes before the first round are the rows of S with an entry: at most n, and none where S is empty
    before = n + 1 if S.nnz else 0
    rounds = 0
    while before > 0:
        ops.amg_pmis_round(S, ST, count, state, flag, isc, left)
        rounds += 1
        now = ops._scan_rows(left, nb)[1]
        if now >= before:
            raise RuntimeError("PMIS round %d decided nothing (%d nodes undecided)" % (rounds, now))
        before = now
    rank, n_c = _ranks(isc, n)
    return state[:n], rank, n_c, rounds


def greedy_device(S):
    """(state, rank, n_c, 0) of the reference's greedy rule (ops.host_greedy_cf, on the host) on the strength pattern: node
    i is coarse iff no coarse c < i has i in S_c; a fine node whose row of S is empty is AMG_FINE0."""
    n, dev = S.shape[0], S.device
    host = sp.csr_matrix((np.ones(S.nnz), S.colidx.cpu().numpy(), S.rowptr.cpu().numpy()), shape=S.shape)
    isc = ops.host_greedy_cf(host)
    empty = np.diff(host.indptr) == 0
    state = np.where(isc != 0, ops.AMG_COARSE, np.where(empty, ops.AMG_FINE0, ops.AMG_FINE)).astype(np.int32)
    d_isc = torch.from_numpy(np.ascontiguousarray(isc, dtype=np.int32)).to(dev)
    rank, n_c = _ranks(d_isc if n else torch.zeros(1, dtype=I32, device=dev), n)
    return torch.from_numpy(state).to(dev), rank, n_c, 0


def split_device(S, split="pmis"):
    if split not in SPLITS:
        raise ValueError("split must be one of %s, got %r" % (SPLITS, split))
    return pmis_device(S) if split == "pmis" else greedy_device(S)


def direct_interpolation_device(A, S, state, rank, n_c=None):
    """P (n x n_c, DeviceCSR) by direct interpolation.  Raises Refused for a fine row whose d_i is zero or not finite.
    n_c: the number of coarse nodes where the caller knows it (two 4-byte reads otherwise)."""
    n = A.shape[0]
    if n_c is None:
        n_c = int(rank[n - 1].item()) + int(state[n - 1].item() == ops.AMG_COARSE) if n else 0
    status = ops.nmg2d_status(A.device)
    P = ops.amg_interp(A, S, state.contiguous(), rank.contiguous(), n_c, status)
    bad = ops.amg_read_status(status)
    if bad is not None:
        raise Refused(*bad)
    return P


def smooth_interpolation_device(A, P, state, rank, omega=1.0, trunc=0.2):
    """One Jacobi step on P: a fine row takes the pattern of (A P)_i and P_ic - (omega AP_ic) / a_ii; entries below
    trunc * (the row's largest) leave and the rest is scaled back to the row sum."""
    omega = float(omega)
    if not np.isfinite(omega):
        raise ValueError("interp_omega must be finite, got %r" % (omega,))
    AP = ops.spgemm(A, P)
    return ops.amg_smooth(A, P, AP, state.contiguous(), rank.contiguous(), omega, _check_unit("interp_trunc", trunc))


def transfer_device(A, theta=0.25, split="pmis", interp_sweeps=1, interp_omega=1.0, interp_trunc=0.2):
    """(P or None, info) of one level: None where the split gives no coarse level (n_c = 0 or n_c = n)."""
    S = strength_device(A, theta)
    state, rank, n_c, rounds = split_device(S, split)
    info = {"n": A.shape[0], "nnz": A.nnz, "n_c": n_c, "rounds": rounds}
    if n_c == 0 or n_c == A.shape[0]:
        return None, info
    P = direct_interpolation_device(A, S, state, rank, n_c)
    for _ in range(int(interp_sweeps)):
        P = smooth_interpolation_device(A, P, state, rank, interp_omega, interp_trunc)
    return P, info


def classical_hierarchy(A, device, *, theta=0.25, split="pmis", interp_sweeps=1, interp_omega=1.0, interp_trunc=0.2,
                        max_levels=10, max_coarse=500, **hierarchy_kw):
    """The Hierarchy of A (SciPy or ops.DeviceCSR) by classical AMG: per level strength, split, direct interpolation and
    interp_sweeps Jacobi steps on P; A_(l+1) = (P^T A) P as Hierarchy forms it.  The coarsening stops at a level of at most
    max_coarse rows, at max_levels grids, or where a split gives n_c = 0 or n_c = n.  H.amg_info: per level n, nnz, and for
    the levels that were split n_c and the PMIS rounds."""
    from .hierarchy import Hierarchy
    if int(max_levels) < 1 or int(interp_sweeps) < 0:
        raise ValueError("max_levels must be >= 1 and interp_sweeps >= 0")
    if split not in SPLITS:
        raise ValueError("split must be one of %s, got %r" % (SPLITS, split))
    device = torch.device(device)
    info = []

    def transfers(l, Al):
        if l + 1 >= int(max_levels) or Al.shape[0] <= int(max_coarse):
            return None
        P, level = transfer_device(Al, theta, split, interp_sweeps, interp_omega, interp_trunc)
        info.append(level)
        return P

    if device.type == "cuda":
        with torch.cuda.device(device):
            H = Hierarchy(as_device_csr(A, device), transfers, device, **hierarchy_kw)
    else:
        H = Hierarchy(as_device_csr(A, device), transfers, device, **hierarchy_kw)
    H.amg_info = [dict(info[l]) if l < len(info) else {"n": lev.n, "nnz": lev.A.nnz, "n_c": None, "rounds": None}
                  for l, lev in enumerate(H.levels)]
    return H


def hierarchy_info(H):
    """Per level n, nnz, n_c and PMIS rounds (None on a level that was not split), and the operator and grid complexity:
    the sums of nnz and of n over the levels by those of the fine level."""
    levels = [dict(d) for d in getattr(H, "amg_info", [{"n": lev.n, "nnz": lev.A.nnz, "n_c": None, "rounds": None}
                                                       for lev in H.levels])]
    nnz0, n0 = max(levels[0]["nnz"], 1), max(levels[0]["n"], 1)
    return {"levels": levels, "operator_complexity": sum(d["nnz"] for d in levels) / nnz0,
            "grid_complexity": sum(d["n"] for d in levels) / n0}
