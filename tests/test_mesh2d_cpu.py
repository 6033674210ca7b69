"""What can be said about the device meshes (learnmultigrid_amd/mesh.py, csrc/mesh2d.hip) without a GPU: the NumPy
twin the GPU tests compare with (tests/mesh2d_ref.py) against the reference's own meshes (goldens g4) and against the
invariants of a refinement, the keyword checks of Mesh2D, and the new symbols of the library."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
import mesh2d_ref as T
from learnmultigrid_amd import Mesh2D, _lib, mesh

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("k", [4, 16])
def test_twin_constructs_the_reference_mesh(k):
    g = load_golden("g4_structured2d_k%d" % k)
    p, conn = T.construct(k, k)
    assert p.dtype == g["p"].dtype and np.array_equal(p, g["p"])            # bit for bit
    assert np.array_equal(conn, g["conn"])


@pytest.mark.parametrize("h_el,v_el", [(4, 4), (5, 3), (16, 16)])
def test_twin_refinement_invariants(h_el, v_el):
    p, conn = T.construct(h_el, v_el)
    n, ne, edges = p.shape[0], conn.shape[0], T.n_edges(conn)
    assert edges == h_el * (v_el + 1) + v_el * (h_el + 1) + h_el * v_el
    for ratios in (None, T.irregular_ratios(edges, 7)):
        q, kids = T.refine(p, conn, ratios)
        assert q.shape[0] == n + edges and kids.shape[0] == 4 * ne
        assert np.array_equal(q[:n], p)
        assert abs(T.areas(q, kids).sum() - T.areas(p, conn).sum()) <= 4 * EPS * ne
        _l, _r, _h, count = T.edges(kids)
        assert count.min() >= 1 and count.max() <= 2
        assert np.array_equal(T.boundary(q.shape[0], kids), T.unit_square_boundary(q))
    assert np.array_equal(T.boundary(n, conn), T.unit_square_boundary(p))


def test_twin_special_meshes():
    p, conn = T.three_on_one_edge()
    assert T.edges(conn)[3].max() == 3 and T.n_edges(conn) == 7
    q, kids = T.refine(p, conn)
    assert q.shape[0] == 5 + 7 and np.array_equal(q[5], [0.5, 0.0])          # the shared edge has one midpoint
    p, conn = T.with_unused_nodes()
    assert sorted(set(range(p.shape[0])) - set(conn.ravel())) == [5, p.shape[0] - 1]
    p, conn = T.l_shape()
    assert conn.shape[0] == 24 and T.boundary(p.shape[0], conn).sum() == 16
    for m in (5, 63, 64):
        p, conn = T.fan(m)
        assert np.unique(conn[conn[:, 0] == 0]).size == m + 1


def test_twin_identity_rows():
    import scipy.sparse as sp
    A = sp.csr_matrix(np.array([[4.0, -1, 0], [-1, 4, -1], [0, -1, 4]]))
    B, r = T.identity_rows(A, [1.0, 2.0, 3.0], np.array([True, False, True]), value=np.array([7.0, 8.0, 9.0]))
    assert np.array_equal(B.toarray(), [[1, 0, 0], [-1, 4, -1], [0, 0, 1]]) and B.nnz == A.nnz
    assert np.array_equal(r, [7.0, 2.0, 9.0])


def test_find_balanced_couple():
    for ne in range(1, 61):
        a, b = mesh.find_balanced_couple(ne)
        assert a * b == ne and a >= 1 and b >= 1, ne
    assert mesh.find_balanced_couple(15) == (5, 3) and mesh.find_balanced_couple(16) == (4, 4)
    assert Mesh2D.find_balanced_couple(100) == (10, 10)
    assert mesh.prime_factors(360) == [2, 2, 2, 3, 3, 5] and mesh.prime_factors(1) == []


def test_keyword_errors_need_no_device(monkeypatch):
    import torch

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    p, conn = T.construct(2, 2)
    for kw in (dict(), dict(ne=0), dict(ne=-3), dict(ne=2.5), dict(p=p), dict(conn=conn),
               dict(p=p.ravel(), conn=conn), dict(p=p, conn=conn[:, :2]), dict(p=p, conn=conn.astype(float)),
               dict(p=np.zeros((3, 3)), conn=conn)):
        with pytest.raises(ValueError):
            Mesh2D(device="cuda:0", **kw)
    # refine: the combinations are refused before the mesh is looked at
    m = Mesh2D.__new__(Mesh2D)
    for kw in (dict(seed=7), dict(ratios=[0.5]), dict(regular=True, seed=1, ratios=[0.5])):
        with pytest.raises(ValueError):
            m.refine(**kw)
    with pytest.raises(ValueError):
        m.refine(False, ratios=[[0.5]])


def test_new_symbols_load_and_answer_without_a_gpu():
    _lib.build()
    L = _lib.lib()
    names = [s for s in _lib.SIGNATURES if s.startswith("lmg_mesh2d_")] + ["lmg_csr_identity_rows"]
    assert len(names) == 10
    for name in names:
        assert hasattr(L, name), name
    assert mesh.limits() >= 32 and Mesh2D.limits() == mesh.limits()
    a = ctypes.c_int32()
    assert L.lmg_mesh2d_limits(None) == -1 and L.lmg_mesh2d_limits(ctypes.byref(a)) == 0 and a.value == mesh.limits()
    # the size rules answer before anything is launched: no device is needed to be told
    assert L.lmg_mesh2d_construct(0, 4, None, None, None, None) == -1
    assert L.lmg_mesh2d_edge_keys(2 ** 31 // 3 + 1, 8, 8, None) == -1
    assert L.lmg_mesh2d_refine(2 ** 31 - 10, 4, 9, 8, 8, 8, 8, 8, None, 16, 16, 16, None) == -1
    assert L.lmg_mesh2d_rows_fill(4, 2, 8, 8, 8, 0, mesh.limits() + 1, 8, None, None) == -4
