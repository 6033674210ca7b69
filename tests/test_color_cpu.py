"""The rules of the "multicolor_device" Gauss-Seidel ordering on their plain-Python twin (tests/color_ref.py): what the
colouring guarantees, on the case matrices the device tests (tests/test_color_gpu.py) repeat integer for integer; the cycle
counts multicolour Gauss-Seidel reaches on the twin's AMG hierarchies; and the new entry points of the built library, as
far as they answer without a device."""
import functools

import numpy as np
import pytest

import amg_cases as C
import color_ref as K
from color_cases import CASES, case_matrices, coloring, complete
from learnmultigrid_amd import _lib


@pytest.mark.parametrize("name", CASES)
def test_colouring_invariants(name):
    A = case_matrices()[name]
    col, nc, rounds = coloring(name)
    G = K.graph(A)
    n = A.shape[0]
    assert col.shape == (n,) and (n == 0 or (col.min() >= 0 and col.max() == nc - 1))
    for i in range(n):
        near = {int(col[j]) for j in G[i]}
        assert int(col[i]) not in near, "an edge joins two nodes of colour %d at node %d" % (col[i], i)
        assert set(range(int(col[i]))) <= near, "node %d of colour %d lacks a neighbour of a colour below" % (i, col[i])
    maxdeg = max((len(set(g)) for g in G), default=0)
    assert nc <= maxdeg + 1 or n == 0
    assert (rounds == 0) == (n == 0)
    rows, ptr = K.schedule(col, nc)
    assert ptr[0] == 0 and ptr[-1] == n and np.all(np.diff(ptr) > 0)
    for c in range(nc):
        part = rows[ptr[c]:ptr[c + 1]]
        assert np.all(col[part] == c) and np.all(np.diff(part) > 0)


def test_known_colour_counts():
    assert coloring("diagonal")[1:] == (1, 1)                      # isolated nodes: colour 0 in the first round
    assert coloring("n1")[1:] == (1, 1)
    assert coloring("n0")[1:] == (0, 0)
    assert coloring("star70")[1] == 2
    assert coloring("complete64")[1:] == (64, 64)
    A = case_matrices()["dirichlet_rows"]
    assert (abs(A) != abs(A.T)).nnz > 0                            # the pattern is unsymmetric


def test_more_than_64_colours_are_refused():
    with pytest.raises(K.Refused) as e:
        K.color(complete(65))
    assert 0 <= e.value.node < 65
    # the node of the smallest key is the one left over
    assert e.value.node == min(range(65), key=lambda i: (K.hash32(i), i))


# ---- cycle counts --------------------------------------------------------------------------------------------------------
JACOBI_COUNTS = {"poisson": 17, "jittered": 20, "renumbered": 22}      # V(2,2) damped Jacobi on the same hierarchies (recorded)


@functools.lru_cache(maxsize=None)
def twin_schedules(name):
    Ps, As, _ = C.twin_hierarchy(name)
    out = []
    for A in As[:len(Ps)]:
        col, nc, _ = K.color(A)
        out.append(K.schedule(col, nc))
    return out


@pytest.mark.parametrize("pair", [("forward", "forward"), ("forward", "backward")], ids=["forward", "symmetric_pair"])
@pytest.mark.parametrize("name", sorted(JACOBI_COUNTS))
def test_cycle_counts_beat_jacobi(name, pair):
    A, b = C.problems()[name]
    Ps, As, _ = C.twin_hierarchy(name)
    assert len(As) >= 3
    hist = K.VCycle(As, Ps, twin_schedules(name), steps=2, gs_sweep=pair).history(b, C.CAP, C.TARGET)
    count = C.cycles_needed(hist)
    print("%s %s: %s cycles" % (name, pair, count))
    assert count is not None and count <= C.CAP
    assert count < JACOBI_COUNTS[name]


# ---- the library ----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lmg_color_select", "lmg_color_blocks", "lmg_color_assign", "lmg_color_twin_count", "lmg_color_twin_fill",
               "lmg_color_twin_refill", "lmg_color_sweep")
ERR_ARG = -1


def test_library_exports_and_refuses_null_arguments():
    """Null pointers and negative sizes answer LMG_ERR_ARG before anything is launched (safe with or without a device)."""
    _lib.build()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    a = np.zeros(8, dtype=np.int32).ctypes.data                   # any valid address: the calls below never reach a launch
    assert L.lmg_color_blocks(0) == 0 and L.lmg_color_blocks(257) == 2 and L.lmg_color_blocks(-1) == 0
    assert L.lmg_color_select(4, None, None, None, None, None, None, None) == ERR_ARG
    assert L.lmg_color_select(-1, a, a, a, a, a, a, None) == ERR_ARG
    assert L.lmg_color_select(4, a, a, a, a, a, None, None) == ERR_ARG
    assert L.lmg_color_assign(4, None, None, None, None, None, None, None, None, None) == ERR_ARG
    assert L.lmg_color_assign(4, a, a, a, a, a, a, a, None, None) == ERR_ARG
    assert L.lmg_color_assign(-1, a, a, a, a, a, a, a, a, None) == ERR_ARG
    assert L.lmg_color_twin_count(1, 1, None, None, None, None, None, None, None, None) == ERR_ARG
    assert L.lmg_color_twin_count(-1, 1, a, a, a, a, a, a, a, None) == ERR_ARG
    assert L.lmg_color_twin_count(1, 65, a, a, a, a, a, a, a, None) == ERR_ARG
    assert L.lmg_color_twin_count(1, 0, a, a, a, a, a, a, a, None) == ERR_ARG
    assert L.lmg_color_twin_fill(1, None, None, None, None, None, None, None, None, None) == ERR_ARG
    assert L.lmg_color_twin_fill(-1, a, a, a, a, a, a, a, a, None) == ERR_ARG
    assert L.lmg_color_twin_refill(64, None, None, None, None) == ERR_ARG
    assert L.lmg_color_twin_refill(-1, a, a, a, None) == ERR_ARG
    assert L.lmg_color_sweep(1, None, None, None, None, None, None, None, 1, 64, None, None, 1, 0, None) == ERR_ARG
    assert L.lmg_color_sweep(-1, a, a, a, a, a, a, a, 1, 64, a, a, 1, 0, None) == ERR_ARG
    assert L.lmg_color_sweep(1, a, a, a, a, a, a, a, 1, 64, a, a, -1, 0, None) == ERR_ARG
    assert L.lmg_color_sweep(1, a, a, a, a, a, a, a, 1, 64, a, a, 1, 2, None) == ERR_ARG
    assert L.lmg_color_sweep(65, a, a, a, a, a, a, a, 1, 64, a, a, 1, 0, None) == ERR_ARG
    # nothing to do: no launch, no device needed
    assert L.lmg_color_select(0, a, a, a, a, a, a, None) == 0
    assert L.lmg_color_sweep(0, a, a, a, a, a, a, a, 0, 0, a, a, 1, 0, None) == 0
    assert L.lmg_color_sweep(1, a, a, a, a, a, a, a, 1, 64, a, a, 0, 0, None) == 0


def test_hierarchy_refuses_the_mode_on_an_ops_module_without_it():
    """An ops module that does not offer build_gs_schedule_device (the CPU stand-in) refuses the mode by name."""
    import types

    from learnmultigrid_amd.hierarchy import Hierarchy
    H = Hierarchy.__new__(Hierarchy)
    H.ops = types.SimpleNamespace()
    H.levels = [types.SimpleNamespace(gs_sched={}, A=None, host_pattern=None)]
    with pytest.raises(ValueError, match="multicolor_device"):
        H.gs_schedule(0, "multicolor_device")
    assert H.levels[0].host_pattern is None
