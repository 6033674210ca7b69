"""Meshes built, refined and indexed on an MI355X (-m gpu): learnmultigrid_amd/mesh.py and csrc/mesh2d.hip against the
NumPy twin (tests/mesh2d_ref.py), the reference's meshes and matrices (goldens g4) and the host constructor
assembly.P1Mesh2D.__init__, which the device topology must equal integer for integer.

Coordinates are compared by their bits, connectivity and graph arrays exactly.  The assembly tolerances are those of
tests/test_assembly_gpu.py (1e-13 stiffness, 1e-15 mass, rtol 1e-12 load) because the same kernel runs on the same graph.

End to end: the cap of 50 cycles was checked on the CPU oracle (oracle/vcycle_ref.HoistedVCycle with the NumPy
transfer_2d, V(2,2), Jacobi at 0.8) before any device run: 7 cycles for the regular hierarchy, 10 for the one whose finest
mesh is refined irregularly with seed 7."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from conftest import load_golden, coo_from                              # noqa: E402
import mesh2d_ref as T                                                  # noqa: E402
from learnmultigrid_amd import Mesh2D, _lib, l2_projection as L2, mesh, ops      # noqa: E402
from learnmultigrid_amd.assembly import P1Mesh2D                        # noqa: E402
from learnmultigrid_amd.solvers import HierarchyMG                      # noqa: E402

DEV = "cuda:0"
STRUCTURED = {"one": 1, "5x3": 15, "25": 25, "64x64": 64 * 64}
GRAPH = ("n2e_ptr", "n2e_elem", "n2e_loc", "rowptr", "colidx")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and torch.equal(torch.from_numpy(a).view(torch.int64), torch.from_numpy(b).view(torch.int64))


def device_mesh(name):
    if name in STRUCTURED:
        return Mesh2D(STRUCTURED[name], device=DEV)
    p, conn = T.CASES[name]()
    return Mesh2D(p=p, conn=conn, device=DEV)


def assert_is_twin(m, p, conn):
    assert m.n_p == p.shape[0] and m.ne == conn.shape[0] and m.get_np() == m.n_p and m.get_ne() == m.ne
    assert same_bits(m.p, p), "coordinates differ from the twin"
    assert np.array_equal(m.conn, conn), "connectivity differs from the twin"


def assert_graph_is_the_hosts(m):
    """from_device against P1Mesh2D.__init__ of the downloaded arrays; twice, for identical tensors."""
    dev, again = P1Mesh2D.from_device(m.px, m.py, m.dconn), m.p1()
    host = P1Mesh2D(m.p, m.conn, DEV)
    assert (dev.n, dev.ne, dev.nnz) == (host.n, host.ne, host.nnz)
    for name in GRAPH:
        d, h = getattr(dev, name), getattr(host, name)
        assert d.dtype == h.dtype and torch.equal(d, h), name
        assert torch.equal(d, getattr(again, name)), name + " (second call)"
    return dev


def refined_like(m, **kw):
    """A second mesh from the same arrays, refined the same way: for the "same bits" check."""
    other = Mesh2D(p=m.p, conn=m.conn, device=DEV)
    return other.refine(**kw)


@pytest.mark.parametrize("k", [4, 16])
def test_construct_is_the_reference_mesh(k):
    g = load_golden("g4_structured2d_k%d" % k)
    m = Mesh2D(k * k, device=DEV)
    assert_is_twin(m, g["p"], g["conn"])
    assert m.get_points() is m.p and m.get_connections() is m.conn and m.get_mesh()[0] is m.p


@pytest.mark.parametrize("name", list(T.CASES))
def test_refine_and_graph_against_the_twin_and_the_host(name):
    p, conn = T.CASES[name]()
    m = device_mesh(name)
    assert_is_twin(m, p, conn)
    dev = assert_graph_is_the_hosts(m)
    if name == "unused":
        rows = np.diff(dev.rowptr.cpu().numpy())
        unused = sorted(set(range(p.shape[0])) - set(conn.ravel()))
        assert len(unused) == 2 and np.all(rows[unused] == 0) and np.all(np.delete(rows, unused) > 0)
    # irregular, from the unrefined mesh
    ratios = T.irregular_ratios(T.n_edges(conn), 7)
    irr = Mesh2D(p=p, conn=conn, device=DEV)
    assert irr.refine(False, seed=7) is irr
    assert_is_twin(irr, *T.refine(p, conn, ratios))
    assert_graph_is_the_hosts(irr)
    byhand = Mesh2D(p=p, conn=conn, device=DEV).refine(False, ratios=ratios)
    assert torch.equal(byhand.px, irr.px) and torch.equal(byhand.py, irr.py) and torch.equal(byhand.dconn, irr.dconn)
    # regular, once and twice
    for _ in range(2):
        twice = refined_like(m)
        p, conn = T.refine(p, conn)
        m.refine()
        assert_is_twin(m, p, conn)
        assert torch.equal(twice.px, m.px) and torch.equal(twice.py, m.py) and torch.equal(twice.dconn, m.dconn)
        assert_graph_is_the_hosts(m)


def test_refine_keywords_on_the_device():
    m = Mesh2D(4, device=DEV)
    with pytest.raises(ValueError):
        m.refine(False, ratios=np.full(3, 0.5))                        # 16 edges
    assert m.n_p == 9 and m.ne == 8                                    # unchanged


def test_row_limit():
    limit = mesh.limits()
    assert limit >= 32
    p, conn = T.fan(limit - 1)
    m = Mesh2D(p=p, conn=conn, device=DEV)
    dev = assert_graph_is_the_hosts(m)
    assert int(dev.rowptr[1]) == limit                                 # the centre row: itself and the ring
    p, conn = T.fan(limit)
    m = Mesh2D(p=p, conn=conn, device=DEV)
    for _ in range(2):
        with pytest.raises(_lib.LmgError, match="capacity"):
            m.p1()
        assert m._p1 is None                                            # no partial result is kept
    with pytest.raises(_lib.LmgError, match="capacity"):
        P1Mesh2D.from_device(m.px, m.py, m.dconn)
    m.refine()                                                          # refinement has no such limit ...
    assert_is_twin(m, *T.refine(p, conn))
    with pytest.raises(_lib.LmgError, match="capacity"):               # ... and the centre keeps its neighbours
        m.p1()


def test_check_refuses_by_element_number():
    p, conn = T.construct(3, 3)
    bad = conn.copy()
    bad[7, 1] = p.shape[0]
    bad[11, 0] = -1
    with pytest.raises(ValueError, match="element 7: a vertex index outside"):
        Mesh2D(p=p, conn=bad, device=DEV)
    bad = conn.copy()
    bad[5, 2] = bad[5, 0]
    bad[9, 1] = bad[9, 2]
    with pytest.raises(ValueError, match="element 5: a repeated vertex"):
        Mesh2D(p=p, conn=bad, device=DEV)
    t = torch.from_numpy(bad.astype(np.int32).ravel()).to(DEV)
    px, py = (torch.from_numpy(np.ascontiguousarray(p[:, k])).to(DEV) for k in (0, 1))
    with pytest.raises(ValueError, match="element 5"):
        P1Mesh2D.from_device(px, py, t)


def test_boundary_nodes():
    m = Mesh2D(16 * 16, device=DEV).refine()
    b = m.boundary_nodes()
    assert b.dtype == torch.bool and b.is_cuda and b.shape == (m.n_p,)
    assert np.array_equal(b.cpu().numpy(), T.unit_square_boundary(m.p))
    assert int(b.sum()) == 4 * 32
    p, conn = T.l_shape()
    m = Mesh2D(p=p, conn=conn, device=DEV)
    assert np.array_equal(m.boundary_nodes().cpu().numpy(), T.boundary(p.shape[0], conn))
    m.refine()
    assert np.array_equal(m.boundary_nodes().cpu().numpy(), T.boundary(m.n_p, m.conn))
    p, conn = T.three_on_one_edge()                                    # the edge of three elements is no boundary edge
    m = Mesh2D(p=p, conn=conn, device=DEV)
    assert np.array_equal(m.boundary_nodes().cpu().numpy(), T.boundary(p.shape[0], conn))


@pytest.mark.parametrize("k", [4, 16])
def test_assembly_and_identity_rows_match_the_reference(k):
    g = load_golden("g4_structured2d_k%d" % k)
    m = Mesh2D(k * k, device=DEV)
    A, M, rhs = m.p1().assemble(load=-1.0)
    assert abs(A.to_scipy() - coo_from(g, "A_free")).max() <= 1e-13
    assert abs(M.to_scipy() - coo_from(g, "M")).max() <= 1e-15
    nnz = A.nnz
    A2, rhs2 = m.dirichlet(A, rhs)
    assert A2 is A and rhs2 is rhs and A.nnz == nnz                    # in place, entries stay stored
    got = A.to_scipy()
    got.eliminate_zeros()
    assert abs(got - coo_from(g, "A")).max() <= 1e-13
    r = rhs.cpu().numpy()
    np.testing.assert_allclose(r, g["rhs"].ravel(), rtol=1e-12)
    b = m.boundary_nodes().cpu().numpy()
    assert b.sum() == 4 * k and np.all(r[b] == 0.0)


def test_identity_rows_with_values_a_mask_and_a_missing_diagonal():
    m = Mesh2D(15, device=DEV)
    A, _M, rhs = m.p1().assemble(mass=False, load=-1.0)
    host, r0 = A.to_scipy(), rhs.cpu().numpy()
    mask = np.zeros(m.n_p, dtype=bool)
    mask[[0, 7, 8, 23]] = True
    value = np.arange(m.n_p, dtype=np.float64) + 0.5
    m.dirichlet(A, rhs, mask=mask, value=torch.from_numpy(value).to(DEV))
    want, wr = T.identity_rows(host, r0, mask, value)
    got = A.to_scipy()
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data, want.data) and np.array_equal(rhs.cpu().numpy(), wr)
    assert abs(got - got.T).max() > 0                                   # columns untouched
    # rows 1 and 2 lack their diagonals: the lower one is named, and nothing is changed
    rowptr = torch.tensor([0, 2, 3, 4], dtype=torch.int32, device=DEV)
    colidx = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=DEV)
    vals = torch.tensor([4.0, -1.0, -1.0, -2.0], dtype=torch.float64, device=DEV)
    B = ops.DeviceCSR(rowptr, colidx, vals.clone(), (3, 3))
    b = torch.ones(3, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="row 1: no stored diagonal"):
        mesh.identity_rows(B, b, torch.tensor([True, True, True]))
    assert torch.equal(B.vals, vals) and torch.equal(b, torch.ones_like(b))
    mesh.identity_rows(B, b, torch.tensor([True, False, False]))
    assert B.vals.tolist() == [1.0, 0.0, -1.0, -2.0] and b.tolist() == [0.0, 1.0, 1.0]


def solve_history(meshes, boundary):
    """V(2,2) with Jacobi at 0.8 on the hierarchy of the meshes (finest first): the residual history."""
    fine = meshes[0].p1() if isinstance(meshes[0], Mesh2D) else meshes[0]
    A, _M, rhs = fine.assemble(mass=False, load=-1.0)
    mesh.identity_rows(A, rhs, boundary)
    Q = L2.mesh_hierarchy_2d("pseudo", meshes)
    mg = HierarchyMG(A.to_scipy(), rhs.cpu().numpy().reshape(-1, 1), Q)
    mg.solve(levels=3, smoother="Jacobi", smooth_steps=2, omega=0.8, smoother_semantics="as_named", max_iterations=50,
             error=1e-8)
    return np.asarray(mg.get_track_res()).ravel(), float(mg.get_residual())


@pytest.mark.parametrize("irregular", [False, True])
def test_end_to_end_mesh_to_solve(irregular):
    m0 = Mesh2D(8 * 8, device=DEV)
    m1 = Mesh2D(p=m0.p, conn=m0.conn, device=DEV).refine()
    m2 = Mesh2D(p=m1.p, conn=m1.conn, device=DEV)
    m2 = m2.refine(False, seed=7) if irregular else m2.refine()
    assert m2.n_p == 33 * 33
    if not irregular:                                                   # 33^2 nodes, not in grid order
        grid = T.construct(32, 32)[0]
        assert not np.array_equal(m2.p, grid) and np.array_equal(np.unique(m2.p, axis=0), np.unique(grid, axis=0))
    hist, last = solve_history([m2, m1, m0], m2.boundary_nodes())
    host = [P1Mesh2D(m.p, m.conn, DEV) for m in (m2, m1, m0)]
    want, _ = solve_history(host, m2.boundary_nodes())
    print("irregular" if irregular else "regular", "cycles", hist.size - 1, "final residual %.3e" % last)
    assert hist.size >= 2 and np.array_equal(hist, want)                # identical topology, identical bits
    assert last <= 1e-8 and hist.size - 1 <= 50
