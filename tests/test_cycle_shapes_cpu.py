"""Host logic of the W- and F-cycles on CPU tensors (no GPU): Hierarchy.cycle(shape=...) with the test-only ops shim
against the CPU restatement of pyamg's cycle shapes (cycle_shapes_ref.ShapeCycle), where the turnaround passes go, and
the keywords the solvers accept."""
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cpu_ops_shim as shim
from cycle_shapes_ref import ShapeCycle, history
from learnmultigrid_amd import problems as P
from learnmultigrid_amd.hierarchy import CYCLE_SHAPES, Hierarchy, cycle_children
from oracle import kernels as K


def _np(t):
    return t.numpy()


def _sp(A):
    return sp.csr_matrix((_np(A.vals), _np(A.colidx), _np(A.rowptr)), shape=A.shape)


def fused_shim(turnaround=True):
    """The shim plus stand-ins of the fused passes (oracle arithmetic, the order of the separate launches) and of the
    turnaround pass (the correcting pass, then the restricting pass); every fused call is recorded."""
    ns = types.SimpleNamespace(**{k: getattr(shim, k) for k in dir(shim) if not k.startswith("__")})
    calls = []
    ns.calls = calls
    ns.FUSED_MAX_SWEEPS = 3
    ns.stencil_smooth_available = lambda A: True
    ns.stencil_smooth_prolong_available = lambda A, P_: True
    ns.stencil_smooth_restrict_available = lambda A, R: True
    ns.stencil_smooth_turnaround_selected = lambda A, P_, R: turnaround

    def smooth(A, x_in, b, omega, sweeps, x_out, r_out=None, prolong=None, restrict=None):
        assert prolong is None or restrict is None
        As = _sp(A)
        bb = _np(b)
        x = np.zeros(A.shape[0]) if x_in is None else _np(x_in).copy()
        if prolong is not None:
            x = K.spmv(_sp(prolong[0]), _np(prolong[1]), x, 1.0, 1.0)
        for _ in range(sweeps):
            x = K.jacobi(As, x, bb, omega)
        _np(x_out)[:] = x
        r, _ = K.residual(As, x, bb)
        if r_out is not None:
            _np(r_out)[:] = r
        if restrict is not None:
            _np(restrict[1])[:] = K.matvec(_sp(restrict[0]), r)
        calls.append(("prolong" if prolong is not None else "restrict" if restrict is not None else "plain", A.shape[0]))

    def turn(A, x_in, b, omega, s_post, s_pre, x_out, prolong, restrict):
        tmp = torch.empty_like(x_out)
        smooth(A, x_in, b, omega, s_post, tmp, prolong=prolong)
        smooth(A, tmp, b, omega, s_pre, x_out, restrict=restrict)
        calls[-2:] = [("turnaround", A.shape[0])]

    ns.stencil_smooth = smooth
    ns.stencil_smooth_turnaround = turn
    return ns


def _problem(m=64, levels=5):
    A, rhs = P.poisson_2d_structured(m)
    return A, rhs, P.geometric_hierarchy_2d(m + 1, levels)


def _run(H, rhs, cycles, shape, smoother="Jacobi", omega=0.8):
    H.levels[0].b.copy_(torch.from_numpy(rhs.ravel().copy()))
    H.ops.zero(H.levels[0].x)
    norms = []
    for _ in range(cycles):
        norms.append(H.residual_norm())
        H.cycle(smoother, 3, omega, shape=shape)
    return np.array(norms), H.levels[0].x.numpy().copy()


def test_shape_names():
    assert CYCLE_SHAPES == ("V", "W", "F")
    assert cycle_children("V") == ("V",) and cycle_children("W") == ("W", "W") and cycle_children("F") == ("F", "V")
    for bad in ("w", "VW", None, "cycle"):
        with pytest.raises(ValueError):
            cycle_children(bad)


@pytest.mark.parametrize("shape", ["V", "W", "F"])
def test_shim_cycles_match_the_restatement(shape):
    A, rhs, hier = _problem()
    H = Hierarchy(A, hier, "cpu", ops_mod=shim)
    got, x = _run(H, rhs, 4, shape)
    want, xw = history(ShapeCycle(A, hier, shape), A, rhs, 4, smoother="Jacobi", steps=3, omega=0.8)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)
    np.testing.assert_allclose(x, xw, rtol=1e-10, atol=1e-12 * np.abs(xw).max())
    if shape == "W":
        hv, _ = history(ShapeCycle(A, hier, "V"), A, rhs, 4, smoother="Jacobi", steps=3, omega=0.8)
        assert want[-1] < 0.9 * hv[-1]                          # the shapes are told apart: W converges faster


def test_shim_gauss_seidel_cycles_match_the_restatement():
    A, rhs, hier = _problem(32, 4)
    for shape in ("W", "F"):
        H = Hierarchy(A, hier, "cpu", ops_mod=shim)
        got, x = _run(H, rhs, 3, shape, smoother="GaussSeidel", omega=1.0)
        want, _ = history(ShapeCycle(A, hier, shape), A, rhs, 3, smoother="GaussSeidel", steps=3)
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)


@pytest.mark.parametrize("shape,levels,count", [("V", 5, 0), ("W", 5, 1 + 2 + 4), ("F", 5, 3), ("W", 3, 1), ("F", 2, 0)])
def test_turnaround_placement_keeps_the_bits(shape, levels, count):
    """The turnaround runs once between every two consecutive visits of a level (W: 2^(l-1) on level l, F: one on every
    level from 1 to L-2) and changes no bit of the history or of the solution."""
    A, rhs, hier = _problem(64, levels)
    on, off = fused_shim(True), fused_shim(False)
    h_on, x_on = _run(Hierarchy(A, hier, "cpu", ops_mod=on), rhs, 3, shape)
    h_off, x_off = _run(Hierarchy(A, hier, "cpu", ops_mod=off), rhs, 3, shape)
    assert np.array_equal(h_on, h_off) and np.array_equal(x_on, x_off)
    turns = [c for c in on.calls if c[0] == "turnaround"]
    assert len(turns) == 3 * count
    assert all(n != A.shape[0] for _, n in turns)              # never on the fine level (one visit per cycle)
    assert len(on.calls) == len(off.calls) - len(turns)        # each replaces two passes
    want, _ = history(ShapeCycle(A, hier, shape), A, rhs, 3, smoother="Jacobi", steps=3, omega=0.8)
    np.testing.assert_allclose(h_on, want, rtol=1e-10, atol=0)


def test_turnaround_waits_for_fused_levels_and_short_smoothing():
    """steps > 3 (two passes per smoothing half) and non-fusable smoothers keep the two separate halves."""
    A, rhs, hier = _problem(64, 5)
    on = fused_shim(True)
    H = Hierarchy(A, hier, "cpu", ops_mod=on)
    H.levels[0].b.copy_(torch.from_numpy(rhs.ravel().copy()))
    H.cycle("Jacobi", 4, 0.8, shape="W")
    assert not [c for c in on.calls if c[0] == "turnaround"]
    on.calls.clear()
    H.cycle("GaussSeidel", 2, 1.0, shape="W")
    assert not on.calls


def test_cycle_rejects_unknown_shapes():
    A, rhs, hier = _problem(32, 3)
    H = Hierarchy(A, hier, "cpu", ops_mod=shim)
    with pytest.raises(ValueError):
        H.cycle("Jacobi", 1, 0.8, shape="X")
