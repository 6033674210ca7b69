"""TEST-ONLY plain-Python restatement of the rules of the multicolour Gauss-Seidel ordering "multicolor_device" (DESIGN.md
section 3, "Multicolour Gauss-Seidel on the device"): the parallel greedy colouring, the schedule, the sequential sweep over a
row list (the update of gs.hip's gs_update_row) and a V-cycle around it.  Written from the rules, node by node, with no care
for speed: what ops.color_device, ops.build_gs_schedule_device and csrc/color.hip are compared with, integer for integer and
bit for bit.  Nothing in learnmultigrid_amd imports this file.

Matrices are SciPy CSR; explicit zeros stay where they are and count as entries of the pattern."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from amg_ref import hash32

MAX_COLORS = 64


class Refused(ValueError):
    def __init__(self, node):
        super().__init__("node %d would need colour %d" % (node, MAX_COLORS))
        self.node = int(node)


def graph(A):
    """Per node the neighbours in G: the pattern of A and A^T without the diagonal (a neighbour may be listed twice)."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    T = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape).T.tocsr()
    return [[int(j) for j in A.indices[A.indptr[i]:A.indptr[i + 1]] if j != i]
            + [int(j) for j in T.indices[T.indptr[i]:T.indptr[i + 1]] if j != i] for i in range(n)]


def color(A):
    """(colour, ncolours, rounds).  A round: every uncoloured node whose key (hash, index) exceeds that of every uncoloured
    neighbour is flagged; every flagged node takes the smallest colour none of its coloured neighbours has.  A node that
    would need colour MAX_COLORS stays uncoloured; the round that then colours nothing raises Refused with the smallest
    such node."""
    G = graph(A)
    n = len(G)
    key = [(hash32(i), i) for i in range(n)]
    col = np.full(n, -1, dtype=np.int32)
    rounds, refused = 0, []
    while np.any(col < 0):
        rounds += 1
        flagged = [i for i in range(n) if col[i] < 0 and all(key[i] > key[j] for j in G[i] if col[j] < 0)]
        done = 0
        for i in flagged:                                           # (no two of them are neighbours: any order)
            used = {int(col[j]) for j in G[i] if col[j] >= 0}
            c = next(c for c in range(MAX_COLORS + 1) if c not in used)
            if c == MAX_COLORS:
                refused.append(i)
            else:
                col[i] = c
                done += 1
        if done == 0:
            if refused:
                raise Refused(min(refused))
            raise RuntimeError("a colouring round coloured nothing")
    return col, int(col.max()) + 1 if n else 0, rounds


def schedule(col, ncolors):
    """(rows ordered by (colour, row), pointers of the colours into them)."""
    rows = np.argsort(col, kind="stable").astype(np.int32)
    ptr = np.zeros(ncolors + 1, dtype=np.int32)
    np.cumsum(np.bincount(col, minlength=ncolors), out=ptr[1:])
    return rows, ptr


def reversed_schedule(rows, ptr):
    return rows[::-1].copy(), (int(ptr[-1]) - ptr[::-1]).astype(np.int32)


def sweep(A, x, b, rows, sweeps=1):
    """`sweeps` sequential walks of the row list, in place on x: rsum over the entries off the diagonal in storage order,
    one rounded product and one rounded sum per entry; diag the last stored entry on the diagonal; x[i] = (b[i] - rsum) /
    diag; a row without a diagonal or with a zero one is left as it is."""
    ip, ix, va = A.indptr, A.indices, A.data
    for _ in range(sweeps):
        for i in rows:
            rsum, diag = 0.0, 0.0
            for k in range(ip[i], ip[i + 1]):
                j = ix[k]
                if j == i:
                    diag = float(va[k])
                else:
                    rsum += float(va[k]) * float(x[j])
            if diag != 0.0:
                x[i] = (float(b[i]) - rsum) / diag
    return x


class VCycle:
    """V(steps, steps) cycles with multicolour Gauss-Seidel on the operators As and transfers Ps (SciPy products, a direct
    solve on the last level).  schedules[l] = (rows, ptr) of level l; gs_sweep: (pre, post) of "forward" | "backward" |
    "symmetric"."""

    def __init__(self, As, Ps, schedules, steps=2, gs_sweep=("forward", "forward")):
        self.As = [sp.csr_matrix(A) for A in As]
        self.Ps = [sp.csr_matrix(P) for P in Ps]
        self.Rs = [sp.csr_matrix(P.T) for P in self.Ps]
        self.fwd = [rows for rows, _ in schedules]
        self.bwd = [rows[::-1].copy() for rows, _ in schedules]
        self.steps, self.pair = steps, gs_sweep
        self.coarse = spla.splu(sp.csc_matrix(self.As[len(self.Ps)]))

    def _smooth(self, l, x, b, direction):
        if direction == "symmetric":
            for _ in range(self.steps):
                sweep(self.As[l], x, b, self.fwd[l])
                sweep(self.As[l], x, b, self.bwd[l])
        else:
            sweep(self.As[l], x, b, self.fwd[l] if direction == "forward" else self.bwd[l], self.steps)

    def cycle(self, x, b, l=0):
        if l == len(self.Ps):
            return self.coarse.solve(b)
        self._smooth(l, x, b, self.pair[0])
        e = self.cycle(np.zeros(self.As[l + 1].shape[0]), self.Rs[l] @ (b - self.As[l] @ x), l + 1)
        x += self.Ps[l] @ e
        self._smooth(l, x, b, self.pair[1])
        return x

    def history(self, b, cap, target):
        """[||b - A x_k||] from x_0 = 0 up to the first norm at or below target * ||b||, at most cap cycles."""
        A = self.As[0]
        b = np.asarray(b, dtype=np.float64).ravel()
        x = np.zeros(A.shape[0])
        hist = [float(np.linalg.norm(b - A @ x))]
        while hist[-1] > target * hist[0] and len(hist) <= cap:
            x = self.cycle(x, b)
            hist.append(float(np.linalg.norm(b - A @ x)))
        return hist
