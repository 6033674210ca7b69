"""The smoothing ops of an operator handle, torch.ops.lmg.operator_* (-m gpu): every launch sequence torch_ops.Operator
takes through smoothing.py -- fused passes and one launch per sweep, the one-pass and the two-launch Chebyshev step, the
wavefront kernel and the level schedule in both directions -- bit for bit against the CPU oracle's sweeps
(oracle.kernels, tests/chebyshev_ref.py), and the caller's x left alone by the ops that return a new vector."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import chebyshev_ref as C                                        # noqa: E402
from learnmultigrid_amd import ops, problems as P, torch_ops    # noqa: E402
from oracle import kernels as K                                  # noqa: E402  (checker only)
from support import dev                                          # noqa: E402

SWEEPS = (0, 1, 3, 4, 7)


def _operator(name):
    """The 5-point operator on 65 x 65 (4225 rows, just above ops.TILED_MIN_ROWS) or 33 x 33 (1089 rows), or the latter
    under a fixed symmetric row / column permutation (no grid order: no stencil twin)."""
    A = K.as_csr(P.poisson_2d_structured({"65": 64, "33": 32, "33_permuted": 32}[name])[0])
    if name == "33_permuted":
        p = np.random.default_rng(11).permutation(A.shape[0])
        A = K.as_csr(A[p][:, p])
    return A


@pytest.fixture(scope="module")
def case():
    """name -> (A, handle, x0, b), created once; the handles are freed at the end."""
    ops.register_torch_ops()
    made = {}

    def get(name):
        if name not in made:
            A = _operator(name)
            rng = np.random.default_rng(5)
            h = torch.ops.lmg.operator_create(dev(A.indptr), dev(A.indices), dev(A.data), A.shape[1])
            made[name] = (A, h, rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0]))
        return made[name]

    yield get
    for _A, h, _x, _b in made.values():
        torch.ops.lmg.operator_free(h)


@pytest.fixture(scope="module")
def jacobi_reference():
    """name -> the oracle's iterates after 0 .. 7 Jacobi sweeps with omega 0.8 (computed once, read only)."""
    made = {}

    def get(name, A, x0, b):
        if name not in made:
            xs = [x0.copy()]
            for _ in range(max(SWEEPS)):
                xs.append(K.jacobi(A, xs[-1], b, 0.8))
            made[name] = xs
        return made[name]
    return get


@pytest.mark.parametrize("sweeps", SWEEPS)
@pytest.mark.parametrize("name,kind", [("65", "tile"), ("33", None)])
def test_operator_jacobi(case, jacobi_reference, name, kind, sweeps):
    """Fused passes of three sweeps on the 65 x 65 operator, one launch per sweep on the 33 x 33 one."""
    A, h, x0, b = case(name)
    assert ops._fused_kind(torch_ops._get(h).A) == kind
    x = dev(x0)
    keep = x.clone()
    got = torch.ops.lmg.operator_jacobi(h, x, dev(b), 0.8, sweeps)
    assert np.array_equal(got.cpu().numpy(), jacobi_reference(name, A, x0, b)[sweeps])
    assert torch.equal(x, keep) and got.data_ptr() != x.data_ptr()


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_operator_chebyshev(case, degree):
    """Degrees up to FUSED_MAX_SWEEPS run as the one tiled pass, degree 4 as two launches per sweep."""
    A, h, x0, b = case("65")
    assert ops.stencil_cheby_available(torch_ops._get(h).A) and ops.FUSED_MAX_SWEEPS == 3
    x = dev(x0)
    keep = x.clone()
    got = torch.ops.lmg.operator_chebyshev(h, x, dev(b), degree, 0.0, 4.0)          # lmax 0: the Gershgorin bound, 2
    assert np.array_equal(got.cpu().numpy(), C.cheby_step(A, x0, b, C.coefficients(2.0, 4.0, degree)))
    assert torch.equal(x, keep)


@pytest.mark.parametrize("sweeps", [1, 3])
@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("name,wavefront", [("65", True), ("33_permuted", False)])
def test_operator_gauss_seidel(case, name, wavefront, direction, sweeps):
    """The wavefront kernel on the grid operator, the level schedule on the permuted one; the second call on the same
    handle sweeps on with what the first one set up (the cached schedule)."""
    A, h, x0, b = case(name)
    assert ops.stencil_gs_available(torch_ops._get(h).A, direction) == wavefront
    n = A.shape[0]
    rows = np.arange(n, dtype=np.int32) if direction == "forward" else np.arange(n - 1, -1, -1, dtype=np.int32)
    op = torch.ops.lmg.operator_gauss_seidel_ if direction == "forward" else torch.ops.lmg.operator_gauss_seidel_backward_
    x, want = dev(x0), x0.copy()
    for call in range(2):
        op(h, x, dev(b), sweeps)
        for _ in range(sweeps):
            K.gs_rows(A, want, b, rows)
        assert np.array_equal(x.cpu().numpy(), want), call
    if not wavefront:
        assert direction in torch_ops._get(h).gs
