"""fp32 cycle operators without a GPU: the C ABI carries the five _f32 entry points, the `values=` / `cycle_values=`
keywords are checked before anything is built, and a hierarchy on matrices without twins (the CPU ops shim) is not
affected by the keyword."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cpu_ops_shim as shim
from learnmultigrid_amd import _lib, ops, problems as P
from learnmultigrid_amd.hierarchy import Hierarchy
from support import header_symbols

NEW = ("lmg_sell_fill_f32", "lmg_sell_sweep_f32", "lmg_dia_fill_f32", "lmg_dia_smooth_f32", "lmg_dia_cheby_f32")


def test_the_five_entry_points_are_declared_bound_and_exported():
    hdr = header_symbols()
    for name in NEW:
        assert name in hdr, name
        assert name in _lib.SIGNATURES, name
    # same argument lists as the fp64 namesakes; the SELL fill takes one more pointer, the flag word
    for name in NEW:
        res, args = _lib.SIGNATURES[name]
        res64, args64 = _lib.SIGNATURES[name[:-4]]
        assert res == res64
        assert args == (args64[:-1] + [ctypes.c_void_p, args64[-1]] if name == "lmg_sell_fill_f32" else args64), name
    _lib.build()
    built = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(built, name), name


def _cpu_matrix():
    A = sp.csr_matrix(P.poisson_2d_structured(8)[0])
    return ops.DeviceCSR.from_scipy(A, "cpu")


@pytest.mark.parametrize("builder", [ops.SellCSR, ops.DiaTwin], ids=["sell", "dia"])
def test_builders_refuse_an_unknown_width(builder):
    with pytest.raises(ValueError, match="f16"):
        builder.from_csr(_cpu_matrix(), values="f16")
    with pytest.raises(ValueError, match="f16"):
        _cpu_matrix().pack(values="f16")


def _problem():
    m = 16
    A, rhs = P.poisson_2d_structured(m)
    return A, rhs, P.geometric_hierarchy_2d(m + 1, 3)


def test_hierarchy_refuses_an_unknown_width_before_any_setup():
    A, _rhs, hier = _problem()
    built = []

    class Plan(shim.SpGEMMPlan):
        def __init__(self, *a, **k):
            built.append("plan")
            super().__init__(*a, **k)
    ns = shim.namespace(SpGEMMPlan=Plan)
    with pytest.raises(ValueError, match="cycle_values"):
        Hierarchy(A, hier, "cpu", ops_mod=ns, cycle_values="f16")
    assert built == []
    Hierarchy(A, hier, "cpu", ops_mod=ns)
    assert built                                                     # (the probe does see a setup that runs)


def test_the_keyword_changes_nothing_without_twins():
    A, rhs, hier = _problem()
    out = {}
    for cv in ("f64", "f32"):
        H = Hierarchy(A, hier, "cpu", ops_mod=shim, cycle_values=cv)
        assert H.cycle_values == cv
        assert all(lev.A.twin_values == "f64" and lev.A.sell is None and lev.A.dia is None for lev in H.levels)
        H.levels[0].b.copy_(torch.from_numpy(rhs.ravel().copy()))
        shim.zero(H.levels[0].x)
        for _ in range(3):
            H.cycle("Jacobi", 2, 0.8)
        out[cv] = (H.levels[0].x.numpy().copy(), [lev.dinv.numpy().copy() for lev in H.levels[1:-1]],
                   H.memory_bytes(), H.cycle_bytes(2), H.twin_bytes())
    assert np.array_equal(out["f64"][0], out["f32"][0]) and np.abs(out["f64"][0]).max() > 0
    for a, b in zip(out["f64"][1], out["f32"][1]):
        assert np.array_equal(a, b)
    assert out["f64"][2:] == out["f32"][2:] and out["f32"][4] == 0
    H32 = Hierarchy(A, hier, "cpu", ops_mod=shim, cycle_values="f32")
    with pytest.raises(ValueError, match="preconditioner"):
        H32.residual_norm()
