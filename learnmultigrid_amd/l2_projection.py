"""L2-projection transfer operators, vectorised: 1-D below, 2-D between triangle meshes in the
second half of the file (the reference has no 2-D path to restate).


Restates learn_multigrid/L2_projection: `L2Projection(type, fine_mesh, coarse_mesh)
.compute_transfer_1d()` (L2Projection.py:26-57) = mesh intersection (Intersection.py:35-80, an
O(ne * ne_c) double loop in the reference) + coupling operator B by 3-point Gauss quadrature on
every intersection segment (CouplingOperator.py:32-69) + mass matrix (MassMatrix.py:61-82), then
    "L2"     Q = M^-1 B                         (L2Projection.py:67-72)
    "pseudo" Q = diag(colsum M)^-1 B            (lumped mass, :74-82)
    "quasi"  Q = B / rowsum(B)                  (:84-90)
Here the segments come from one sorted merge of the two node sets (O(n log n)) and B, M are
assembled with array operations; results agree with the reference's to rounding
(tests/test_l2_projection.py against goldens g2 / g3).  Returned sparse (CSR); the reference
returns the same matrix dense."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

# Quadrature(3) of the reference (assembly/Quadrature.py:52-66), 14-digit constants included
_GP = np.array([0.11270166537926, 0.50000000000000, 0.88729833462074])
_GW = np.array([0.27777777777778, 0.44444444444444, 0.27777777777778])


def mass_matrix_1d(x):
    """P1 mass matrix of the 1-D mesh with nodes x (MassMatrix.compute_mass_1d)."""
    x = np.asarray(x, dtype=np.float64)
    h = np.diff(x)
    # loc_m[i, j] = h * sum_k phi_i(p_k) phi_j(p_k) w_k  with phi = (1 - p, p)
    phi = np.stack([1.0 - _GP, _GP])                      # (2, 3)
    ref = np.einsum("ik,jk,k->ij", phi, phi, _GW)         # (2, 2)
    n = x.size
    i = np.arange(n - 1)
    rows = np.concatenate([i, i, i + 1, i + 1])
    cols = np.concatenate([i, i + 1, i, i + 1])
    vals = np.concatenate([h * ref[0, 0], h * ref[0, 1], h * ref[1, 0], h * ref[1, 1]])
    return sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()


def coupling_operator_1d(x_fine, x_coarse):
    """B (n_fine x n_coarse): integral of fine basis x coarse basis over every intersection of a
    fine with a coarse element."""
    xf = np.asarray(x_fine, dtype=np.float64)
    xc = np.asarray(x_coarse, dtype=np.float64)
    union = np.union1d(xf, xc)                            # Intersection.py:57
    xa, xb = union[:-1], union[1:]
    mid = 0.5 * (xa + xb)
    fe = np.clip(np.searchsorted(xf, mid, side="right") - 1, 0, xf.size - 2)    # fine element of each segment
    ce = np.clip(np.searchsorted(xc, mid, side="right") - 1, 0, xc.size - 2)
    phys = xa[:, None] + _GP[None, :] * (xb - xa)[:, None]                      # g_function
    fr = (phys - xf[fe][:, None]) / (xf[fe + 1] - xf[fe])[:, None]              # inv_g_function
    cr = (phys - xc[ce][:, None]) / (xc[ce + 1] - xc[ce])[:, None]
    pf = np.stack([1.0 - fr, fr], axis=1)                 # (nseg, 2, 3)
    pc = np.stack([1.0 - cr, cr], axis=1)
    loc = np.einsum("sik,sjk,k->sij", pf, pc, _GW) * (xb - xa)[:, None, None]
    rows = np.stack([fe, fe, fe + 1, fe + 1], axis=1).ravel()
    cols = np.stack([ce, ce + 1, ce, ce + 1], axis=1).ravel()
    return sp.coo_matrix((loc.reshape(-1, 4).ravel(), (rows, cols)), shape=(xf.size, xc.size)).tocsr()


def transfer_1d(kind, x_fine, x_coarse):
    """Q of L2Projection(kind, fine, coarse).compute_transfer_1d(); kind in L2 | pseudo | quasi."""
    B = coupling_operator_1d(x_fine, x_coarse)
    if kind == "quasi":
        rs = np.asarray(B.sum(axis=1)).ravel()
        return sp.csr_matrix(sp.diags(1.0 / rs) @ B)
    M = mass_matrix_1d(x_fine)
    if kind == "pseudo":
        lumped = np.asarray(M.sum(axis=0)).ravel()
        return sp.csr_matrix(sp.diags(1.0 / lumped) @ B)
    if kind == "L2":
        return sp.csr_matrix(spla.spsolve(sp.csc_matrix(M), sp.csc_matrix(B)))
    raise ValueError("Invalid order %r (L2 | pseudo | quasi)" % (kind,))


def transfer_1d_device(kind, x_fine, x_coarse, device):
    """The same Q on an MI355X (csrc/l2proj.hip: one thread per fine node, segments by binary search,
    rows in CSR): kind in B | pseudo | quasi ("L2" is a dense M^-1 B: use transfer_1d).  Returns an
    ops.DeviceCSR; nodes must be strictly increasing."""
    import torch
    from . import ops, _lib
    code = {"B": 0, "pseudo": 1, "quasi": 2}.get(kind)
    if code is None:
        raise ValueError("device transfer: kind must be B | pseudo | quasi, got %r" % (kind,))
    xf = np.ascontiguousarray(np.asarray(x_fine, dtype=np.float64).ravel())
    xc = np.ascontiguousarray(np.asarray(x_coarse, dtype=np.float64).ravel())
    if xf.size < 2 or xc.size < 2 or np.any(np.diff(xf) <= 0) or np.any(np.diff(xc) <= 0):
        raise ValueError("node coordinates must be strictly increasing (at least two nodes per mesh)")
    dxf, dxc = torch.from_numpy(xf).to(device), torch.from_numpy(xc).to(device)
    nf, nc = xf.size, xc.size
    L = _lib.lib()
    s = torch.cuda.current_stream(dxf.device).cuda_stream
    rownnz = torch.empty(nf, dtype=torch.int32, device=device)
    _lib.check(L.lmg_l2_coupling_count(nf, nc, dxf.data_ptr(), dxc.data_ptr(), rownnz.data_ptr(), s), "lmg_l2_coupling_count")
    rowptr = torch.empty(nf + 1, dtype=torch.int32, device=device)
    ops.exclusive_scan_i32(rownnz, rowptr)
    nnz = int(rowptr[-1])
    colidx = torch.empty(nnz, dtype=torch.int32, device=device)
    vals = torch.empty(nnz, dtype=torch.float64, device=device)
    _lib.check(L.lmg_l2_coupling_fill(code, nf, nc, dxf.data_ptr(), dxc.data_ptr(), rowptr.data_ptr(), colidx.data_ptr(),
                                      vals.data_ptr(), s), "lmg_l2_coupling_fill")
    return ops.DeviceCSR(rowptr, colidx, vals, (nf, nc))


# ---- 2-D: two P1 triangle meshes that need not be nested ---------------------------------------------------------
# The reference stops at a stub here (L2Projection.compute_transfer_2d; Intersection.find_intersections2d assumes four
# children per coarse element), so the rules are this project's own and the host functions below are their statement;
# csrc/l2proj2d.hip follows the same rules on the device.
#   pairs    (fine element e, coarse element c) whose bounding boxes overlap, found through a uniform cell grid over the
#            coarse mesh -- never all against all
#   clip     e against the three edges of c by Sutherland-Hodgman, c taken counter-clockwise (by the sign of its
#            determinant), inside = side >= 0, a crossing = P + (Q - P) * s_P / (s_P - s_Q); at most POLY vertices
#   drop     the polygon's area (fan from vertex 0, |det| / 2 each) must exceed area_tol * min(|T_e|, |T_c|): elements
#            that only touch leave polygons of rounding size, which would add entries of rounding size to B
#   rule     the reference's 2-D quadrature (Quadrature.py:87-97) on every fan triangle with det != 0, exact for the
#            quadratic phi_i * phi_j; barycentric coordinates in e and in c by the determinant formula
POLY = 7
_Q2 = np.array([[1.0 / 6.0, 1.0 / 6.0], [1.0 / 6.0, 2.0 / 3.0], [2.0 / 3.0, 1.0 / 6.0]])


def _mesh(p, conn):
    p = np.ascontiguousarray(p, dtype=np.float64)
    conn = np.ascontiguousarray(conn, dtype=np.int64)
    if p.ndim != 2 or p.shape[1] != 2 or conn.ndim != 2 or conn.shape[1] != 3 or not conn.size:
        raise ValueError("a triangle mesh is p of shape (n, 2) and conn of shape (ne, 3)")
    if conn.min() < 0 or conn.max() >= p.shape[0]:
        raise ValueError("conn names a node outside p")
    return p, conn


def _det3(a, b, c):
    """(b - a) x (c - a) on the last axis of (..., 2) arrays."""
    return (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (c[..., 0] - a[..., 0]) * (b[..., 1] - a[..., 1])


def lumped_mass_2d(p, conn):
    """Column sums of the P1 mass matrix: sum of |det_e| / 6 over the elements of each node, e ascending."""
    p, conn = _mesh(p, conn)
    t = p[conn]
    out = np.zeros(p.shape[0])
    np.add.at(out, conn.ravel(), np.repeat(np.abs(_det3(t[:, 0], t[:, 1], t[:, 2])) / 6.0, 3))
    return out


def mass_matrix_2d(p, conn):
    """P1 mass matrix of a triangle mesh: |det_e| / 24 * (1 + delta_ij) per element."""
    p, conn = _mesh(p, conn)
    t = p[conn]
    loc = (np.abs(_det3(t[:, 0], t[:, 1], t[:, 2])) / 24.0)[:, None, None] * (np.ones((3, 3)) + np.eye(3))
    rows = np.repeat(conn, 3, axis=1).ravel()
    cols = np.tile(conn, (1, 3)).ravel()
    M = sp.coo_matrix((loc.ravel(), (rows, cols)), shape=(p.shape[0],) * 2).tocsr()
    M.sum_duplicates()
    M.sort_indices()
    return M


def _expand(lo_x, hi_x, lo_y, hi_y):
    """Every (owner, ix, iy) with lo_x <= ix <= hi_x, lo_y <= iy <= hi_y, owners ascending."""
    w = hi_x - lo_x + 1
    cnt = w * (hi_y - lo_y + 1)
    owner = np.repeat(np.arange(cnt.size), cnt)
    k = np.arange(owner.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return owner, lo_x[owner] + k % w[owner], lo_y[owner] + k // w[owner]


def candidate_pairs_2d(p_f, conn_f, p_c, conn_c, cells=None):
    """(e, c) of every fine / coarse element pair whose bounding boxes overlap (closed boxes: touching counts), ordered
    by e, then c.  cells: cells per direction of the grid over the coarse mesh's bounding box (None: about one cell per
    two coarse elements).  The work is proportional to the pairs the cells bring together."""
    p_f, conn_f = _mesh(p_f, conn_f)
    p_c, conn_c = _mesh(p_c, conn_c)
    tf, tc = p_f[conn_f], p_c[conn_c]
    flo, fhi, clo, chi = tf.min(axis=1), tf.max(axis=1), tc.min(axis=1), tc.max(axis=1)
    org, end = clo.min(axis=0), chi.max(axis=0)
    nc = int(cells) if cells else max(1, int(np.ceil(np.sqrt(conn_c.shape[0] / 2.0))))
    inv = np.where(end > org, nc / np.where(end > org, end - org, 1.0), 0.0)

    def cell(v):
        return np.clip(np.floor((v - org) * inv), 0, nc - 1).astype(np.int64)

    c0, c1, f0, f1 = cell(clo), cell(chi), cell(flo), cell(fhi)
    c_id, ix, iy = _expand(c0[:, 0], c1[:, 0], c0[:, 1], c1[:, 1])
    key = iy * nc + ix
    order = np.lexsort((c_id, key))
    key, c_id = key[order], c_id[order]
    cellptr = np.searchsorted(key, np.arange(nc * nc + 1))
    live = np.flatnonzero(np.all(fhi >= org, axis=1) & np.all(flo <= end, axis=1))
    k_e, ix, iy = _expand(f0[live, 0], f1[live, 0], f0[live, 1], f1[live, 1])
    fkey = iy * nc + ix
    cnt = cellptr[fkey + 1] - cellptr[fkey]
    slot = np.repeat(np.arange(fkey.size), cnt)
    ent = np.repeat(cellptr[fkey], cnt) + np.arange(slot.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    e, c, ix, iy = live[k_e[slot]], c_id[ent], ix[slot], iy[slot]
    # a pair met in several cells counts in the first cell the two cell ranges share; then the boxes themselves decide
    keep = (ix == np.maximum(f0[e, 0], c0[c, 0])) & (iy == np.maximum(f0[e, 1], c0[c, 1]))
    keep &= np.all(flo[e] <= chi[c], axis=1) & np.all(clo[c] <= fhi[e], axis=1)
    e, c = e[keep], c[keep]
    order = np.lexsort((c, e))
    return e[order], c[order]


def _clip(F, C):
    """Sutherland-Hodgman on arrays: the triangles F (k, 3, 2) against the counter-clockwise triangles C (k, 3, 2).
    Returns (poly (k, POLY, 2), n (k,)): the vertices and their count."""
    k = F.shape[0]
    idx = np.arange(k)
    poly = np.zeros((k, POLY, 2))
    poly[:, :3] = F
    n = np.full(k, 3)
    for edge in range(3):
        a, b = C[:, edge], C[:, (edge + 1) % 3]
        s = (b[:, None, 0] - a[:, None, 0]) * (poly[:, :, 1] - a[:, None, 1]) \
            - (b[:, None, 1] - a[:, None, 1]) * (poly[:, :, 0] - a[:, None, 0])
        out = np.zeros_like(poly)
        m = np.zeros(k, dtype=np.int64)

        def emit(mask, v):
            w = np.flatnonzero(mask & (m < POLY))
            out[w, m[w]] = v[w]
            m[w] += 1

        for i in range(POLY):
            act = i < n
            if not act.any():
                break
            prev = np.where(i == 0, n - 1, i - 1)
            P, sP, Q, sQ = poly[idx, prev], s[idx, prev], poly[:, i], s[:, i]
            with np.errstate(divide="ignore", invalid="ignore"):
                X = P + (Q - P) * (sP / (sP - sQ))[:, None]
            emit(act & ((sQ >= 0) != (sP >= 0)), X)
            emit(act & (sQ >= 0), Q)
        poly, n = out, m
    return poly, n


def coupling_operator_2d(p_f, conn_f, p_c, conn_c, area_tol=1e-14, cells=None):
    """B (n_fine x n_coarse), B_ij = integral of fine basis i x coarse basis j over the intersections of the fine with
    the coarse elements, by the rules at the head of this section.  Sorted CSR; a kept pair enters all nine products."""
    p_f, conn_f = _mesh(p_f, conn_f)
    p_c, conn_c = _mesh(p_c, conn_c)
    e, c = candidate_pairs_2d(p_f, conn_f, p_c, conn_c, cells)
    F, C = p_f[conn_f[e]], p_c[conn_c[c]]
    det_f, det_c = _det3(F[:, 0], F[:, 1], F[:, 2]), _det3(C[:, 0], C[:, 1], C[:, 2])
    ccw = np.where((det_c < 0)[:, None, None], C[:, [0, 2, 1]], C)
    poly, n = _clip(F, ccw)
    v0 = poly[:, 0]
    area = np.zeros(e.size)
    loc = np.zeros((e.size, 3, 3))
    for t in range(1, POLY - 1):
        va, vb = poly[:, t], poly[:, t + 1]
        det = np.where(t + 1 < n, _det3(v0, va, vb), 0.0)
        area += np.abs(det) / 2.0
        for xi, eta in _Q2:
            x = v0 + (va - v0) * xi + (vb - v0) * eta
            with np.errstate(divide="ignore", invalid="ignore"):
                lf = np.stack([_det3(x, F[:, 1], F[:, 2]), _det3(F[:, 0], x, F[:, 2]), _det3(F[:, 0], F[:, 1], x)], 1) / det_f[:, None]
                lc = np.stack([_det3(x, C[:, 1], C[:, 2]), _det3(C[:, 0], x, C[:, 2]), _det3(C[:, 0], C[:, 1], x)], 1) / det_c[:, None]
            w = np.abs(det) / 6.0
            loc += np.where((det != 0)[:, None, None], w[:, None, None] * lf[:, :, None] * lc[:, None, :], 0.0)
    keep = area > area_tol * np.minimum(np.abs(det_f), np.abs(det_c)) / 2.0
    rows = np.repeat(conn_f[e[keep]], 3, axis=1).ravel()
    cols = np.tile(conn_c[c[keep]], (1, 3)).ravel()
    B = sp.coo_matrix((loc[keep].ravel(), (rows, cols)), shape=(p_f.shape[0], p_c.shape[0])).tocsr()
    B.sum_duplicates()
    B.sort_indices()
    return B


def _scale_rows(B, d):
    """B with row i divided by d[i]; rows without entries stay empty whatever d holds."""
    B = sp.csr_matrix(B, copy=True)
    B.data = B.data / np.repeat(d, np.diff(B.indptr))
    return B


def transfer_2d(kind, p_f, conn_f, p_c, conn_c, area_tol=1e-14, cells=None):
    """Q between two triangle meshes; kind in B | L2 | pseudo | quasi, with the 1-D meanings: "pseudo" divides row i of
    B by the lumped fine mass, "quasi" by the row's sum, "L2" solves with the fine mass matrix (dense, host only)."""
    if kind not in ("B", "L2", "pseudo", "quasi"):
        raise ValueError("Invalid order %r (B | L2 | pseudo | quasi)" % (kind,))
    B = coupling_operator_2d(p_f, conn_f, p_c, conn_c, area_tol, cells)
    if kind == "B":
        return B
    if kind == "quasi":
        return _scale_rows(B, np.asarray(B.sum(axis=1)).ravel())
    if kind == "pseudo":
        return _scale_rows(B, lumped_mass_2d(p_f, conn_f))
    return sp.csr_matrix(spla.spsolve(sp.csc_matrix(mass_matrix_2d(p_f, conn_f)), sp.csc_matrix(B)))


DEVICE_KINDS_2D = {"B": 0, "pseudo": 1, "quasi": 2}


def _device_kind_2d(kind):
    if kind == "L2":
        raise ValueError("device transfer: \"L2\" (M^-1 B, dense) is host only -- use transfer_2d(\"L2\", ...)")
    code = DEVICE_KINDS_2D.get(kind)
    if code is None:
        raise ValueError("device transfer: kind must be B | pseudo | quasi, got %r" % (kind,))
    return code


def _device_mesh_2d(mesh, device):
    from .assembly import P1Mesh2D
    if isinstance(mesh, P1Mesh2D):
        return mesh
    from .mesh import Mesh2D
    if isinstance(mesh, Mesh2D):
        return mesh.p1()
    if device is None:
        raise ValueError("a mesh given as (p, conn) needs device=")
    p, conn = _mesh(*mesh)
    if max(p.shape[0], conn.shape[0]) >= 2 ** 31 - 1:
        raise ValueError("mesh too large for int32 indices")
    return P1Mesh2D(p, conn, device)


def limits_2d():
    """(candidates per fine element, distinct columns per row) the kernels of csrc/l2proj2d.hip hold."""
    import ctypes
    from . import _lib
    a, b = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.lib().lmg_l2p2d_limits(ctypes.byref(a), ctypes.byref(b)), "lmg_l2p2d_limits")
    return a.value, b.value


def candidates_2d_device(fine, coarse, cells=None):
    """(candptr, cand): for every fine element the coarse elements whose bounding boxes overlap its own, ascending and
    without duplicates, as CSR of int32 on the device -- candidate_pairs_2d there.  cells: cells per direction of the
    grid over the coarse mesh (None: about one cell per two coarse elements); the result does not depend on it."""
    import torch
    from . import ops, _lib
    from .ops import _p, _s
    L, dev = _lib.lib(), fine.device
    I32, I64 = torch.int32, torch.int64
    nc = int(cells) if cells else max(1, int(np.ceil(np.sqrt(coarse.ne / 2.0))))
    with torch.cuda.device(dev):
        # the grid: origin, far corner and cells per unit length, kept on the device
        used = coarse.conn.long()
        lo = torch.stack([coarse.px[used].min(), coarse.py[used].min()])
        hi = torch.stack([coarse.px[used].max(), coarse.py[used].max()])
        span = hi - lo
        inv = torch.where(span > 0, nc / torch.where(span > 0, span, torch.ones_like(span)), torch.zeros_like(span))
        grid = torch.cat([lo, hi, inv]).contiguous()
        cmesh = (coarse.ne, _p(coarse.px), _p(coarse.py), _p(coarse.conn))
        # coarse elements into the cells their boxes overlap: count, scan, fill, order
        cnt = torch.empty(coarse.ne, dtype=I32, device=dev)
        _lib.check(L.lmg_l2p2d_cell_count(*cmesh, _p(grid), nc, _p(cnt), _s()), "lmg_l2p2d_cell_count")
        ptr = torch.empty(coarse.ne + 1, dtype=I32, device=dev)
        ops.exclusive_scan_i32(cnt, ptr)
        total = int(cnt.sum(dtype=I64))
        keys = torch.empty(total, dtype=I64, device=dev)
        _lib.check(L.lmg_l2p2d_cell_fill(*cmesh, _p(grid), nc, total, _p(ptr), _p(keys), _s()), "lmg_l2p2d_cell_fill")
        keys, _ = torch.sort(keys)
        cellptr = torch.searchsorted(keys, torch.arange(nc * nc + 1, dtype=I64, device=dev) << 32).to(I32)
        cellent = (keys & 0xFFFFFFFF).to(I32)
        # fine elements: the candidates of each, as CSR
        fmesh = (fine.ne, _p(fine.px), _p(fine.py), _p(fine.conn))
        tail = (_p(grid), nc, _p(cellptr), _p(cellent))
        cnt = torch.empty(fine.ne, dtype=I32, device=dev)
        _lib.check(L.lmg_l2p2d_cand_count(*fmesh, *cmesh, *tail, _p(cnt), _s()), "lmg_l2p2d_cand_count")
        candptr = torch.empty(fine.ne + 1, dtype=I32, device=dev)
        ops.exclusive_scan_i32(cnt, candptr)
        pairs, most = (int(v) for v in torch.stack([cnt.sum(dtype=I64), cnt.max().to(I64)]).cpu())
        cand = torch.empty(pairs, dtype=I32, device=dev)
        _lib.check(L.lmg_l2p2d_cand_fill(*fmesh, *cmesh, *tail, pairs, most, _p(candptr), _p(cand), _s()),
                   "lmg_l2p2d_cand_fill (%d candidates for one fine element)" % most)
    return candptr, cand


def rows_2d_device(code, fine, coarse, candptr, cand, area_tol=1e-14):
    """The rows of B (code 0), "pseudo" (1) or "quasi" (2) from the candidate lists, as ops.DeviceCSR."""
    import torch
    from . import ops, _lib
    from .ops import _p, _s
    L, dev = _lib.lib(), fine.device
    with torch.cuda.device(dev):
        args = (fine.n, fine.ne, _p(fine.px), _p(fine.py), _p(fine.conn), _p(fine.n2e_ptr), _p(fine.n2e_elem),
                _p(fine.n2e_loc), coarse.n, coarse.ne, _p(coarse.px), _p(coarse.py), _p(coarse.conn), _p(candptr), _p(cand),
                float(area_tol))
        rownnz = torch.empty(fine.n, dtype=torch.int32, device=dev)
        _lib.check(L.lmg_l2p2d_rows_count(*args, _p(rownnz), _s()), "lmg_l2p2d_rows_count")
        rowptr = torch.empty(fine.n + 1, dtype=torch.int32, device=dev)
        ops.exclusive_scan_i32(rownnz, rowptr)
        nnz, most = (int(v) for v in torch.stack([rownnz.sum(dtype=torch.int64), rownnz.max().to(torch.int64)]).cpu())
        colidx = torch.empty(nnz, dtype=torch.int32, device=dev)
        vals = torch.empty(nnz, dtype=torch.float64, device=dev)
        _lib.check(L.lmg_l2p2d_rows_fill(code, *args, nnz, most, _p(rowptr), _p(colidx), _p(vals), _s()),
                   "lmg_l2p2d_rows_fill (a row of more than %d columns)" % (most - 1))
    return ops.DeviceCSR(rowptr, colidx, vals, (fine.n, coarse.n))


def transfer_2d_device(kind, fine, coarse, area_tol=1e-14, device=None, cells=None):
    """transfer_2d on an MI355X (csrc/l2proj2d.hip): kind in B | pseudo | quasi.  fine, coarse: assembly.P1Mesh2D,
    mesh.Mesh2D (through its p1()), or (p, conn) with device=.  Returns an ops.DeviceCSR (n_fine, n_coarse) with sorted columns.  A fine element with more
    candidates, or a row with more columns, than limits_2d() raises _lib.LmgError: nothing is truncated.  cells: see
    candidates_2d_device."""
    code = _device_kind_2d(kind)
    fine, coarse = _device_mesh_2d(fine, device), _device_mesh_2d(coarse, device)
    if fine.device != coarse.device:
        raise ValueError("the two meshes live on different devices")
    candptr, cand = candidates_2d_device(fine, coarse, cells)
    return rows_2d_device(code, fine, coarse, candptr, cand, area_tol)


def mesh_hierarchy_2d(kind, meshes, device=None, area_tol=1e-14):
    """[Q_0, Q_1, ...]: one transfer per consecutive pair of meshes (fine first), computed on the device and returned as
    SciPy CSR -- what HierarchyMG / SemiGeometricMG(hierarchy=...) take; Hierarchy canonicalises its transfers on the
    host, so each Q crosses the bus once, like the learned ones (learned_q2d.define_hierarchy)."""
    _device_kind_2d(kind)
    meshes = [_device_mesh_2d(m, device) for m in meshes]
    if len(meshes) < 2:
        raise ValueError("a hierarchy needs at least two meshes")
    return [transfer_2d_device(kind, f, c, area_tol).to_scipy() for f, c in zip(meshes[:-1], meshes[1:])]
