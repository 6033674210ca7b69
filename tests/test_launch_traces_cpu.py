"""The smoothing paths launch what they launched before smoothing.py and torch_ops.py were split off (no GPU): every ops
call of Hierarchy.cycle, DistributedVCycle.cycle and the operator handles of torch.ops.lmg on the ops shims -- its name,
its flags, the buffers it reads and writes -- against the traces recorded on the commit before the split
(tests/golden/launch_traces.json, written by tools/launch_traces.py; tests/launch_trace.py says what a trace line holds).
The krylov part -- fgmres, block_fgmres, block_pcg and Multigrid.solve_many -- was recorded on the commit before the drivers came
to share their Givens recurrence, their chunk loop and the graph capture."""
import os

import pytest

import launch_trace
from conftest import ROOT


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "launch_traces.json")) as f:
        return launch_trace.load(f)


@pytest.mark.parametrize("part", launch_trace.PARTS)
def test_launch_traces_equal_the_recorded_ones(golden, part):
    got = getattr(launch_trace, part + "_traces")()
    want = {k: v for k, v in golden.items() if k.startswith(part + " ")}
    assert sorted(got) == sorted(want)
    for case in sorted(want):
        assert got[case] == want[case], case


def test_the_trace_sees_a_changed_flag_a_swapped_buffer_and_a_dropped_launch():
    """The wrapper itself: what the comparison above relies on."""
    import types
    import torch
    calls = []
    ns = types.SimpleNamespace(csr_jacobi=lambda A, x_in, b, omega, x_out: calls.append("j"),
                               stencil_smooth=lambda A, x_in, b, omega, sweeps, x_out, r_out=None: calls.append("s"),
                               stencil_smooth_available=lambda A: True)
    A = types.SimpleNamespace(shape=(4, 4), rowptr=None)
    x, tmp, b = torch.zeros(4), torch.zeros(4), torch.zeros(4)

    def run(f):
        tr = launch_trace.Tracer(ns)
        for t, name in ((x, "X"), (tmp, "T"), (b, "b")):
            tr.name(t, name)
        f(tr.ops)
        return tr.log

    base = run(lambda o: (o.stencil_smooth_available(A), o.stencil_smooth(A, None, b, 0.8, 3, tmp), o.csr_jacobi(A, tmp, b, 0.8, x)))
    assert base == ["stencil_smooth A=4x4 x_in=None b=b omega=0.8 sweeps=3 x_out=T r_out=None",
                    "csr_jacobi A=4x4 x_in=T b=b omega=0.8 x_out=X"]
    assert calls == ["s", "j"]                                          # the wrapped functions still run
    assert run(lambda o: (o.stencil_smooth(A, None, b, 0.8, 3, tmp, None), o.csr_jacobi(A, tmp, b, 0.8, x))) == base
    assert run(lambda o: (o.stencil_smooth(A, x, b, 0.8, 3, tmp), o.csr_jacobi(A, tmp, b, 0.8, x))) != base      # x_in
    assert run(lambda o: (o.stencil_smooth(A, None, b, 0.8, 2, tmp), o.csr_jacobi(A, tmp, b, 0.8, x))) != base   # sweeps
    assert run(lambda o: (o.stencil_smooth(A, None, b, 0.8, 3, tmp, x), o.csr_jacobi(A, tmp, b, 0.8, x))) != base  # r_out
    assert run(lambda o: (o.stencil_smooth(A, None, b, 0.8, 3, x), o.csr_jacobi(A, x, b, 0.8, tmp))) != base     # buffers
    assert run(lambda o: (o.csr_jacobi(A, tmp, b, 0.8, x), o.stencil_smooth(A, None, b, 0.8, 3, tmp))) != base   # order
    assert run(lambda o: o.stencil_smooth(A, None, b, 0.8, 3, tmp)) != base                                      # dropped
