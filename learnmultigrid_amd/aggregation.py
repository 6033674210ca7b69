"""Smoothed-aggregation AMG setup on the device (csrc/sa.hip): from a matrix and one near-nullspace candidate to a Hierarchy.

What a pyamg user gets from `pyamg.smoothed_aggregation_solver(A, B)`, in stages that all run in parallel:

    S         = symmetric_strength_device(A, theta)          symmetric strength of connection
    agg, ...  = aggregate_device(S)                          aggregates around MIS-2 roots (not pyamg's sequential pass)
    T, Bc     = tentative_device(agg, n_agg, B)              tentative prolongator of one candidate, and the coarse candidate
    P         = smooth_prolongator_device(A, T, omega)       one Jacobi step on T (ops.spgemm for A T, the step of amg.hip)
    H         = sa_hierarchy(A, device)                      the level loop; every A_(l+1) = (P^T A) P is formed once, by
                                                             Hierarchy, and neither P nor a candidate crosses the bus

Systems (csrc/nsp.hip): nodes of block_size unknowns and up to six candidates, pyamg's BSR matrix with B of shape (n, k):

    C         = condense_device(A, block_size)               one entry per node block, its Frobenius norm; S and agg from C
    X         = candidates_device(B, n, block_size, device)  (n, k); None: ones, or the block_size unit translations
    T, Bc     = tentative_block_device(agg, n_agg, bs, X)    two rounds of Cholesky-QR per aggregate; Bc (k n_agg x k) is the
                                                             candidate block of the next level, whose block size is k

The rules are DESIGN.md section 3, "Smoothed aggregation setup" and "Smoothed aggregation for systems"; tests/sa_ref.py and
tests/nsp_ref.py restate them in plain Python and the kernels give the same integers and bits.  There is no CPU path: every
stage is a launch on the device that holds A.
"""
import numpy as np
import torch

from . import ops
from .amg import Refused, _check_unit, as_device_csr
from .ops import DeviceCSR, F64, I32


def _pattern(rp, cj, shape):
    return DeviceCSR(rp, cj, torch.ones(cj.numel(), dtype=F64, device=cj.device), shape)


def _check_omega(omega):
    omega = float(omega)
    if not np.isfinite(omega):
        raise ValueError("omega must be finite, got %r" % (omega,))
    return omega


def symmetric_strength_device(A, theta=0.0):
    """S, the symmetric strength pattern of the DeviceCSR A as a DeviceCSR with values 1.0 (columns in A's order): j is
    strong in row i iff a_ij a_ij >= theta^2 |a_ii a_jj| with a_ij, a_ii, a_jj non-zero.  A node with an empty row is
    isolated."""
    if A.shape[0] != A.shape[1]:
        raise ValueError("the strength of connection needs a square matrix, got %s" % (A.shape,))
    return _pattern(*ops.sa_strength(A, _check_unit("theta", theta)), A.shape)


def graph_device(S):
    """G, the aggregation graph of the strength pattern S as a sorted DeviceCSR with values 1.0: an edge {i, j} where
    j in S_i or i in S_j and neither node is isolated."""
    return _pattern(*ops.sa_graph(S, S.transpose()), S.shape)


def mis2_device(S, G):
    """(state, rank, n_agg, rounds): the MIS-2 roots of G.  state: int32 per node (ops.SA_ROOT, SA_COVERED, SA_ISOLATED);
    rank[i]: the number of roots below i, for a root its aggregate.  The host reads one count per round -- the nodes still
    undecided -- so the setup cannot be captured into a graph."""
    n, dev = S.shape[0], S.device
    state, t1, flag, c1, isr = (torch.empty(max(n, 1), dtype=I32, device=dev) for _ in range(5))
    ops.sa_mis2_init(S, state, isr)
    nb = ops.sa_blocks(n)
    left = torch.zeros(max(nb, 1), dtype=I32, device=dev)
    # the undecided nodes before the first round are the rows of S with an entry: at most n, and none where S is empty
    before = n + 1 if S.nnz else 0
    rounds = 0
    while before > 0:
        ops.sa_mis2_round(G, state, t1, flag, c1, isr, left)
        rounds += 1
        now = ops._scan_rows(left, nb)[1]
        if now >= before:
            raise RuntimeError("MIS-2 round %d decided nothing (%d nodes undecided)" % (rounds, now))
        before = now
    rank, n_agg = ops._scan_rows(isr, n)
    return state[:n], rank[:n], n_agg, rounds


def aggregate_device(S, parts=None):
    """(agg, n_agg, rounds) of the strength pattern S: agg[i] is the aggregate of node i (int32, -1 for an isolated node),
    rounds the MIS-2 rounds.  parts: a dict that receives G and the states."""
    n, dev = S.shape[0], S.device
    G = graph_device(S)
    state, rank, n_agg, rounds = mis2_device(S, G)
    a1, a2 = (torch.empty(max(n, 1), dtype=I32, device=dev) for _ in range(2))
    ops.sa_assign(G, state.contiguous(), rank.contiguous(), a1, a2)
    if parts is not None:
        parts.update(G=G, state=state)
    return a2[:n], n_agg, rounds


def candidate_device(B, n, device):
    """The candidate as an fp64 vector of n entries on `device`; None: ones."""
    if B is None:
        return torch.ones(n, dtype=F64, device=device)
    if not isinstance(B, torch.Tensor):
        B = torch.from_numpy(np.ascontiguousarray(np.asarray(B, dtype=np.float64).reshape(-1)))
    B = B.to(device=device, dtype=F64).reshape(-1).contiguous()
    if B.numel() != n:
        raise ValueError("the candidate B must have one entry per row: %d, got %d" % (n, B.numel()))
    return B


def condense_device(A, block_size):
    """C, the condensed matrix of the node blocks of the DeviceCSR A (N x N, N = n / block_size): c_IJ the Frobenius norm
    of block (I, J), an entry wherever the block stores one.  block_size 1: A itself."""
    bs = _check_block(block_size, A.shape[0])
    if A.shape[0] != A.shape[1]:
        raise ValueError("the condensation needs a square matrix, got %s" % (A.shape,))
    return A if bs == 1 else ops.nsp_condense(A, bs)


def _check_block(block_size, n):
    bs = int(block_size)
    if bs != block_size or bs < 1:
        raise ValueError("block_size must be an integer >= 1, got %r" % (block_size,))
    if n % bs:
        raise ValueError("block_size %d does not divide the %d rows" % (bs, n))
    return bs


def _check_rank_tol(rank_tol):
    rank_tol = float(rank_tol)
    if not np.isfinite(rank_tol) or rank_tol <= 0.0:
        raise ValueError("rank_tol must be finite and positive, got %r" % (rank_tol,))
    return rank_tol


def candidates_device(B, n, block_size, device):
    """The candidates as a contiguous fp64 (n, k) tensor on `device`, 1 <= k <= 6.  B: a vector of n, an (n, 1) or an
    (n, k) array; None: ones for block_size 1, else the block_size unit translations (B[i, i % block_size] = 1)."""
    bs = _check_block(block_size, n)
    if B is None:
        if bs == 1:
            return torch.ones(n, 1, dtype=F64, device=device)
        if bs > ops.NSP_MAX_CANDIDATES:
            raise ValueError("block_size %d needs %d unit translations, more than the %d candidates supported: pass B"
                             % (bs, bs, ops.NSP_MAX_CANDIDATES))
        X = np.zeros((n, bs))
        X[np.arange(n), np.arange(n) % bs] = 1.0
        return torch.from_numpy(X).to(device)
    if not isinstance(B, torch.Tensor):
        B = torch.from_numpy(np.ascontiguousarray(np.asarray(B, dtype=np.float64)))
    if B.dim() <= 1 or (B.dim() == 2 and B.shape[1] == 1):
        return candidate_device(B, n, device).reshape(n, 1)
    if B.dim() != 2 or B.shape[0] != n:
        raise ValueError("the candidates B must have one row per row of A: %d, got %s" % (n, tuple(B.shape)))
    if not 1 <= B.shape[1] <= ops.NSP_MAX_CANDIDATES:
        raise ValueError("at most %d candidates are supported, got %d" % (ops.NSP_MAX_CANDIDATES, B.shape[1]))
    return B.to(device=device, dtype=F64).contiguous()


def tentative_block_device(agg, n_agg, block_size, X, rank_tol=1e-12):
    """(T, Bc) of the candidates X (n x k) on aggregates of nodes of block_size unknowns (agg: per node): two rounds of
    Cholesky-QR per aggregate.  T (n x k n_agg DeviceCSR): k entries per row of an aggregated node, the row of Q;
    Bc (k n_agg x k): the blocks R' R.  Raises Refused("candidate", row) for an aggregate whose Gram matrix has a pivot
    that is not finite or not above rank_tol g_cc -- fewer rows than candidates, or candidates that are locally dependent --
    with row = block_size * (its smallest node); of several, the smallest row of the first round that refuses."""
    status = torch.full((2,), -1, dtype=torch.int64, device=X.device)
    T, Bc = ops.nsp_tentative(agg.contiguous(), n_agg, block_size, X, _check_rank_tol(rank_tol), status)
    words = status.cpu()
    for r in range(2):
        bad = ops.amg_read_status(words[r:r + 1])
        if bad is not None:
            if bad[0] != "candidate":
                raise RuntimeError("the members of aggregate %d are not listed in ascending order" % bad[1])
            raise Refused(*bad)
    return T, Bc


def tentative_device(agg, n_agg, B):
    """(T, Bc): T (n x n_agg DeviceCSR) with T_ij = B_i / Bc_j for i in aggregate j, Bc_j the 2-norm of B over the
    aggregate (members in ascending order).  Raises Refused("candidate", row) where that norm is zero or not finite."""
    status = ops.nmg2d_status(B.device)
    T, Bc = ops.sa_tentative(agg.contiguous(), n_agg, B, status)
    bad = ops.amg_read_status(status)
    if bad is not None:
        if bad[0] != "candidate":
            raise RuntimeError("the members of aggregate %d are not listed in ascending order" % bad[1])
        raise Refused(*bad)
    return T, Bc


def jacobi_scale(A, omega=4.0 / 3.0):
    """s = omega / rho with rho = ops.csr_gershgorin(A), the bound max_i sum_j |a_ij| / |a_ii| of the spectrum of D^-1 A:
    one 8-byte read."""
    out = torch.zeros(1, dtype=F64, device=A.device)
    ops.csr_gershgorin(A, out)
    return float(np.float64(_check_omega(omega)) / np.float64(out.item()))


def smooth_prolongator_device(A, T, omega=4.0 / 3.0):
    """P_ic = T_ic - (s (A T)_ic) / a_ii on the pattern of (A T)_i, s = jacobi_scale(A, omega); empty rows of T stay
    empty.  The Jacobi step of the classical setup (ops.amg_smooth) with every aggregated row fine and no truncation."""
    state = ops.sa_row_states(T)
    # (the step reads the rank of coarse rows only, and there are none)
    return ops.amg_smooth(A, T, ops.spgemm(A, T), state, state, jacobi_scale(A, omega), 0.0)


def transfer_device(A, B, theta=0.0, omega=4.0 / 3.0, block_size=1, rank_tol=1e-12):
    """(P or None, Bc or None, info) of one level: None where the aggregation gives no coarse level (n_agg = 0 or the
    number of nodes).  B: a vector with block_size 1 runs the single-candidate path (Bc a vector); an (n, k) tensor, or any
    B with block_size > 1, the path of csrc/nsp.hip: strength and aggregates of the condensed matrix, the tentative
    prolongator of k candidates (Bc: k n_agg x k, the candidates of the next level, whose block size is k)."""
    bs = _check_block(block_size, A.shape[0])
    scalar = bs == 1 and B.dim() == 1
    S = symmetric_strength_device(A if scalar else condense_device(A, bs), theta)
    agg, n_agg, rounds = aggregate_device(S)
    info = {"n": A.shape[0], "nnz": A.nnz, "n_agg": n_agg, "rounds": rounds}
    if n_agg == 0 or n_agg == S.shape[0]:
        return None, None, info
    if scalar:
        T, Bc = tentative_device(agg, n_agg, B)
    else:
        T, Bc = tentative_block_device(agg, n_agg, bs, B.reshape(A.shape[0], -1), rank_tol)
    return smooth_prolongator_device(A, T, omega), Bc, info


def sa_hierarchy(A, device, *, theta=0.0, B=None, omega=4.0 / 3.0, block_size=1, rank_tol=1e-12, max_levels=10,
                 max_coarse=500, **hierarchy_kw):
    """The Hierarchy of A (SciPy or ops.DeviceCSR) by smoothed aggregation: per level the symmetric strength pattern, MIS-2
    aggregates, the tentative prolongator of the candidate (B on the fine level, default ones; the Bc of the level above
    below it) and one Jacobi step on it; A_(l+1) = (P^T A) P as Hierarchy forms it.  The coarsening stops at a level of at
    most max_coarse rows, at max_levels grids, or where the aggregation gives n_agg = 0 or n_agg = n.  H.amg_info: per level
    n, nnz, and for the levels that were aggregated n_agg (aggregates, not coarse unknowns), the MIS-2 rounds, block_size
    and candidates.

    Systems: block_size = bs > 1 makes the unknowns bs I .. bs I + bs - 1 one node; strength and aggregates are those of
    the condensed matrix (condense_device).  B may be a vector of n, an (n, 1) or an (n, k) array, k <= 6: the tentative
    prolongator of k candidates is tentative_block_device, and the level loop carries (candidates, block size) down: the
    Bc of the level above and k.  B None: ones for block_size 1, else the bs unit translations.  One candidate on block
    size 1 runs the single-candidate path and gives its bits.  rank_tol: the Cholesky pivot below which an aggregate is
    refused (amg.Refused), relative to the Gram diagonal."""
    from .hierarchy import Hierarchy
    if int(max_levels) < 1:
        raise ValueError("max_levels must be >= 1")
    theta, omega, rank_tol = _check_unit("theta", theta), _check_omega(omega), _check_rank_tol(rank_tol)
    device = torch.device(device)
    # (candidates (n x k), block size) of the level at hand: bs on the fine level, k below it; checked before any launch
    cand = [candidates_device(B, A.shape[0], block_size, device), int(block_size)]
    info = []

    def build():
        dA = as_device_csr(A, device)

        def transfers(l, Al):
            if l + 1 >= int(max_levels) or Al.shape[0] <= int(max_coarse):
                return None
            X, bs = cand
            k = X.shape[1]
            P, Bc, level = transfer_device(Al, X.reshape(-1) if k == 1 and bs == 1 else X, theta, omega, bs, rank_tol)
            info.append(dict(level, block_size=bs, candidates=k))
            if Bc is not None:
                cand[:] = [Bc.reshape(-1, k), k]
            return P

        return Hierarchy(dA, transfers, device, **hierarchy_kw)

    if device.type == "cuda":
        with torch.cuda.device(device):
            H = build()
    else:
        H = build()
    H.amg_info = [dict(info[l]) if l < len(info) else {"n": lev.n, "nnz": lev.A.nnz, "n_agg": None, "rounds": None}
                  for l, lev in enumerate(H.levels)]
    return H


def hierarchy_info(H):
    """Per level n, nnz, n_agg and MIS-2 rounds (None on a level that was not aggregated; an aggregated level also has its
    block_size and candidates), and the operator and grid complexity: the sums of nnz and of n over the levels by those of
    the fine level."""
    levels = [dict(d) for d in getattr(H, "amg_info", [{"n": lev.n, "nnz": lev.A.nnz, "n_agg": None, "rounds": None}
                                                       for lev in H.levels])]
    nnz0, n0 = max(levels[0]["nnz"], 1), max(levels[0]["n"], 1)
    return {"levels": levels, "operator_complexity": sum(d["nnz"] for d in levels) / nnz0,
            "grid_complexity": sum(d["n"] for d in levels) / n0}
