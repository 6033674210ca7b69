"""Triangle meshes built, refined and indexed on the device (csrc/mesh2d.hip): the first stage of the reference's 2-D
workflow -- Mesh2D(ne), mesh.refine(regular), then assembly and the identity rows of the boundary
(learn_multigrid/mesh/Mesh2D.py:27-160, test/thesis_structured_2d.py:380-414).

The rules ("Meshes"): a slot s = 3 e + k is the directed edge conn[e][k] -> conn[e][(k + 1) % 3];
slots with the same end nodes form one undirected edge, whose head is its smallest slot.  The reference numbers a
midpoint when its loop first meets the edge, that is, in the order of the head slots; an edge met once is a boundary
edge.  tests/mesh2d_ref.py states the same in NumPy.  The mesh graph follows assembly.P1Mesh2D.__init__, which stays
the host statement and the oracle of the tests.

torch does the sorts and searches between the kernels; per stage one small read (a count, a status word) crosses the
bus.  Nothing here falls back to the host: without the library or a GPU the calls raise."""
import ctypes
import math

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .ops import DeviceCSR, F64, I32, _p, _s

I64 = torch.int64
RULES = {1: "a vertex index outside the mesh", 2: "a repeated vertex", 3: "no stored diagonal"}
RATIO_LOW, RATIO_HIGH = 0.3, 0.7        # irregular refinement: the point sits at r in [0.3, 0.7) of its edge (:113-115)


def limits():
    """Distinct columns a row of the mesh graph may hold (a node with more neighbours raises _lib.LmgError)."""
    a = ctypes.c_int32()
    check(_lib.lib().lmg_mesh2d_limits(ctypes.byref(a)), "lmg_mesh2d_limits")
    return a.value


def prime_factors(m):
    """The prime factors of m >= 1, ascending, with multiplicity."""
    out, f = [], 2
    while f * f <= m:
        while m % f == 0:
            out.append(f)
            m //= f
        f += 1 if f == 2 else 2
    if m > 1:
        out.append(m)
    return out


def find_balanced_couple(ne):
    """(h_el, v_el) with h_el * v_el == ne, as Mesh2D.find_balanced_couple (:42-61): the root of a square; otherwise the
    prime factors are dealt out from the largest down, each to the side whose product is smaller (ties: the first)."""
    ne = int(ne)
    if ne < 1:
        raise ValueError("ne must be at least 1")
    root = math.isqrt(ne)
    if root * root == ne:
        return root, root
    a = b = 1
    for f in reversed(prime_factors(ne)):
        if b < a:
            b *= f
        else:
            a *= f
    return a, b


def _check_sizes(n, ne):
    if n < 1 or ne < 1:
        raise ValueError("a mesh needs at least one node and one element")
    if n >= 2 ** 31 - 1 or 3 * ne >= 2 ** 31 - 1:
        raise ValueError("mesh too large for int32 indices (n = %d, 3 * ne = %d)" % (n, 3 * ne))


def _status(dev):
    return torch.full((1,), -1, dtype=I64, device=dev)


def _refusal(status, what):
    """ValueError naming the first offender and its rule, if the stage refused (one read back)."""
    word = int(status.item())
    if word != -1:
        raise ValueError("%s %d: %s" % (what, word >> 8, RULES.get(word & 0xFF, "rule %d" % (word & 0xFF))))


def check_device(n, conn):
    """Every index inside [0, n) and no element with a repeated vertex; ValueError naming the lowest element otherwise."""
    ne = conn.numel() // 3
    _check_sizes(n, ne)
    with torch.cuda.device(conn.device):
        st = _status(conn.device)
        check(_lib.lib().lmg_mesh2d_check(n, ne, _p(conn), _p(st), _s(conn)), "lmg_mesh2d_check")
        _refusal(st, "element")


def edges_device(n, conn, mask=None):
    """(head, is_head): per slot the head slot of its edge and the flag "this slot is a head", int32 on the device.
    mask: a zeroed uint8 tensor of n entries that gets 1 on the nodes of the boundary edges."""
    ne, dev = conn.numel() // 3, conn.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        keys = torch.empty(3 * ne, dtype=I64, device=dev)
        check(L.lmg_mesh2d_edge_keys(ne, _p(conn), _p(keys), _s(conn)), "lmg_mesh2d_edge_keys")
        keys, slot = torch.sort(keys, stable=True)
        head = torch.empty(3 * ne, dtype=I32, device=dev)
        is_head = torch.empty(3 * ne, dtype=I32, device=dev)
        check(L.lmg_mesh2d_edge_runs(n, ne, _p(keys), _p(slot), _p(head), _p(is_head), _p(mask), _s(conn)),
              "lmg_mesh2d_edge_runs")
    return head, is_head


def topology_device(n, conn):
    """(n2e_ptr, n2e_elem, n2e_loc, rowptr, colidx) of assembly.P1Mesh2D for a checked mesh, built on the device."""
    ne, dev = conn.numel() // 3, conn.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        nodes, order = torch.sort(conn, stable=True)
        n2e_ptr = torch.searchsorted(nodes, torch.arange(n + 1, dtype=I32, device=dev)).to(I32)
        elem = torch.empty(3 * ne, dtype=I32, device=dev)
        loc = torch.empty(3 * ne, dtype=I32, device=dev)
        check(L.lmg_mesh2d_n2e_fill(ne, _p(order), _p(elem), _p(loc), _s(conn)), "lmg_mesh2d_n2e_fill")
        del nodes, order
        rownnz = torch.empty(n, dtype=I32, device=dev)
        check(L.lmg_mesh2d_rows_count(n, ne, _p(conn), _p(n2e_ptr), _p(elem), _p(rownnz), _s(conn)), "lmg_mesh2d_rows_count")
        rowptr = torch.empty(n + 1, dtype=I32, device=dev)
        ops.exclusive_scan_i32(rownnz, rowptr)
        nnz, most = (int(v) for v in torch.stack([rownnz.sum(dtype=I64), rownnz.max().to(I64)]).cpu())
        if nnz >= 2 ** 31 - 1:
            raise ValueError("mesh graph too large for int32 indices (%d entries)" % nnz)
        colidx = torch.empty(nnz, dtype=I32, device=dev)
        check(L.lmg_mesh2d_rows_fill(n, ne, _p(conn), _p(n2e_ptr), _p(elem), nnz, most, _p(rowptr), _p(colidx), _s(conn)),
              "lmg_mesh2d_rows_fill (a node with more than %d neighbours and itself)" % (most - 1))
    return n2e_ptr, elem, loc, rowptr, colidx


def identity_rows(A, rhs, mask, value=None):
    """Rows i of the DeviceCSR A with mask[i] become identity rows in place (columns untouched: A != A^T afterwards, as
    in the reference), rhs[i] = 0 or value[i].  A masked row without a stored diagonal: ValueError naming the lowest,
    and nothing is changed."""
    n, dev = A.shape[0], A.vals.device
    if A.shape[0] != A.shape[1]:
        raise ValueError("identity rows need a square matrix")
    if any(getattr(A, t) is not None for t in ("packed", "patterns", "sell", "stencil", "dia")):
        raise ValueError("the matrix was packed already: apply the identity rows first")
    mask = torch.as_tensor(mask).to(dev)
    if mask.numel() != n or (rhs is not None and rhs.numel() != n) or (value is not None and value.numel() != n):
        raise ValueError("mask, rhs and value need one entry per row")
    if rhs is not None and (rhs.dtype != F64 or not rhs.is_contiguous() or rhs.device != dev):
        raise TypeError("rhs must be a contiguous float64 tensor on the matrix's device")
    if value is not None:
        value = torch.as_tensor(value, dtype=F64).to(dev).contiguous()
    mask = (mask != 0).to(torch.uint8).contiguous()
    with torch.cuda.device(dev):
        st = _status(dev)
        check(_lib.lib().lmg_csr_identity_rows(n, _p(A.rowptr), _p(A.colidx), _p(A.vals), _p(mask), _p(value), _p(rhs),
                                               _p(st), _s(A.vals)), "lmg_csr_identity_rows")
        _refusal(st, "row")
    return A, rhs


class Mesh2D:
    """Mesh2D(ne) -- ne squares on the unit square, two triangles each -- or Mesh2D(p=, conn=) from triangles, like the
    reference's class, with the arrays living on an MI355X.  .p (n_p, 2) and .conn (ne, 3) are host copies fetched on
    first use; .ne counts the triangles, .n_p the nodes.  px, py, dconn: the device arrays (conn flat, int32).
    embedding(), plotting and the 1-D mesh classes are not provided."""

    def __init__(self, ne=0, p=None, conn=None, device=None):
        given = p is not None and conn is not None and np.size(p) != 0 and np.size(conn) != 0
        if given:
            p = np.asarray(p, dtype=np.float64)
            c = np.asarray(conn)
            if p.ndim != 2 or p.shape[1] != 2 or c.ndim != 2 or c.shape[1] != 3:
                raise ValueError("a mesh is p (n, 2) and conn (ne, 3), got %s and %s" % (p.shape, c.shape))
            if not np.issubdtype(c.dtype, np.integer):
                raise ValueError("conn must hold integers")
            if c.size and (c.min() < -2 ** 31 or c.max() >= 2 ** 31):
                raise ValueError("conn does not fit int32")
            _check_sizes(p.shape[0], c.shape[0])
        else:
            if (p is not None and np.size(p) != 0) or (conn is not None and np.size(conn) != 0):
                raise ValueError("triangles need both p and conn")
            if int(ne) != ne or ne < 1:
                raise ValueError("Mesh2D needs ne >= 1 squares, or triangles (p, conn)")
            h_el, v_el = find_balanced_couple(ne)
            _check_sizes((h_el + 1) * (v_el + 1), 2 * h_el * v_el)
        # ---- nothing above touches a device ----
        _lib.lib()
        if device is None:
            if not torch.cuda.is_available():
                raise _lib.LmgError("no MI355X visible (torch.cuda.is_available() is False); there is no CPU fallback")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = dev = torch.device(device)
        self._p = self._conn = self._boundary = self._p1 = None
        with torch.cuda.device(dev):
            if given:
                self.px = torch.from_numpy(np.ascontiguousarray(p[:, 0])).to(dev)
                self.py = torch.from_numpy(np.ascontiguousarray(p[:, 1])).to(dev)
                self.dconn = torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32).ravel()).to(dev)
                check_device(p.shape[0], self.dconn)
            else:
                n = (h_el + 1) * (v_el + 1)
                self.px = torch.empty(n, dtype=F64, device=dev)
                self.py = torch.empty(n, dtype=F64, device=dev)
                self.dconn = torch.empty(6 * h_el * v_el, dtype=I32, device=dev)
                check(_lib.lib().lmg_mesh2d_construct(h_el, v_el, _p(self.px), _p(self.py), _p(self.dconn), _s(self.px)),
                      "lmg_mesh2d_construct")

    # ---- the reference's attributes and getters ----
    @property
    def n_p(self):
        return int(self.px.numel())

    @property
    def ne(self):
        return int(self.dconn.numel() // 3)

    @property
    def p(self):
        if self._p is None:
            self._p = torch.stack([self.px, self.py], dim=1).cpu().numpy()
        return self._p

    @property
    def conn(self):
        if self._conn is None:
            self._conn = self.dconn.cpu().numpy().reshape(-1, 3).astype(np.int64)
        return self._conn

    def get_points(self):
        return self.p

    def get_connections(self):
        return self.conn

    def get_ne(self):
        return self.ne

    def get_np(self):
        return self.n_p

    def get_mesh(self):
        return self.p, self.conn

    # ---- refinement ----
    def refine(self, regular=True, *, seed=None, ratios=None):
        """Every triangle into four, in place (returns self).  regular: the points are the midpoints.  Otherwise the
        point of the edge that gets node n + j sits at r_j * p[left] + (1 - r_j) * p[right], left -> right the edge's
        head slot, r_j = ratios[j], or 0.3 + 0.4 * RandomState(seed).rand(edges)[j]: the draws of the reference's loop
        under np.random.seed(seed), in its order."""
        if regular and (seed is not None or ratios is not None):
            raise ValueError("a regular refinement takes neither seed nor ratios")
        if ratios is not None:
            ratios = np.ascontiguousarray(ratios, dtype=np.float64)
            if ratios.ndim != 1:
                raise ValueError("ratios: one value per edge expected")
        n, ne, dev = self.n_p, self.ne, self.device
        L = _lib.lib()
        with torch.cuda.device(dev):
            head, is_head = edges_device(n, self.dconn)
            rank = torch.empty(3 * ne + 1, dtype=I32, device=dev)
            ops.exclusive_scan_i32(is_head, rank)
            edges = int(is_head.sum(dtype=I64))
            if n + edges >= 2 ** 31 - 1:
                raise ValueError("refined mesh too large for int32 indices (%d nodes)" % (n + edges))
            ratio = None
            if not regular:
                if ratios is None:
                    ratios = RATIO_LOW + (RATIO_HIGH - RATIO_LOW) * np.random.RandomState(seed).rand(edges)
                if ratios.shape[0] != edges:
                    raise ValueError("ratios: %d values for %d edges" % (ratios.shape[0], edges))
                ratio = torch.from_numpy(ratios).to(dev)
            px = torch.empty(n + edges, dtype=F64, device=dev)
            py = torch.empty(n + edges, dtype=F64, device=dev)
            conn = torch.empty(12 * ne, dtype=I32, device=dev)
            check(L.lmg_mesh2d_refine(n, ne, edges, _p(self.px), _p(self.py), _p(self.dconn), _p(head), _p(rank), _p(ratio),
                                      _p(px), _p(py), _p(conn), _s(px)), "lmg_mesh2d_refine")
        self.px, self.py, self.dconn = px, py, conn
        self._p = self._conn = self._boundary = self._p1 = None
        return self

    # ---- what assembly needs ----
    def boundary_nodes(self):
        """Device bool tensor: node i is an end of an edge that belongs to one element only."""
        if self._boundary is None:
            with torch.cuda.device(self.device):
                mask = torch.zeros(self.n_p, dtype=torch.uint8, device=self.device)
                edges_device(self.n_p, self.dconn, mask)
            self._boundary = mask.bool()
        return self._boundary

    def p1(self):
        """The assembly.P1Mesh2D of this mesh, its graph built on the device; cached until the next refine."""
        if self._p1 is None:
            from .assembly import P1Mesh2D
            self._p1 = P1Mesh2D.from_device(self.px, self.py, self.dconn, checked=True)
        return self._p1

    def dirichlet(self, A, rhs, mask=None, value=None):
        """identity_rows(A, rhs, ...) on the boundary nodes (or on `mask`); returns (A, rhs), changed in place."""
        return identity_rows(A, rhs, self.boundary_nodes() if mask is None else mask, value)

    @staticmethod
    def limits():
        return limits()

    find_balanced_couple = staticmethod(find_balanced_couple)
