"""Every CPU stand-in of learnmultigrid_amd.ops against the kernel it stands for (-m gpu): the cases of
tests/stand_in_parity.py, each run through the stand-in on CPU tensors and through ops on device copies of the same host
arrays, every tensor argument compared -- bit for bit, or within the bound the case derives.  A stand-in that writes another
slice, reads what the kernel leaves unread, treats a masked column or a zero denominator differently, or sums a local block
in another order than it is stored fails here, where the CPU tests built on it would go on passing.

Two kernels every cycle launches and no stand-in wraps get their direct tests at the end: vmul's claim to the bits of the
first Jacobi sweep is a case of the registry; csr_gs_rows runs against the oracle's row sweep."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import stand_in_parity as SP                                         # noqa: E402
from learnmultigrid_amd import ops                                   # noqa: E402
from oracle import kernels as K                                      # noqa: E402  (checker only)
from support import DEV                                              # noqa: E402

PARAMETERS = SP.parameters()


def synchronize(what):
    """Wait for the device; a fault ends the session, so that nothing more is started on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit("the device reported an error after %s (%s): nothing more is run on it" % (what, err), returncode=3)


@pytest.mark.parametrize("op,case", PARAMETERS, ids=["%s-%s" % (op, c.label) for op, c in PARAMETERS])
def test_stand_in_and_kernel_agree(op, case):
    entry = SP.REGISTRY[op]
    inputs = case.inputs()
    stand_ins = SP.implementations(op, entry.only)
    assert stand_ins, op
    if case.raises is not None:                                      # a refusal: on the host, on both sides
        with pytest.raises(case.raises):
            case.run(SP.Side(ops, DEV), inputs)
        for nsname, ns in stand_ins:
            with pytest.raises(case.raises):
                case.run(SP.Side(ns, "cpu"), inputs)
        return
    device = SP.Side(ops, DEV)
    try:
        case.run(device, inputs)
    except SP.Refused as why:
        pytest.skip(str(why))
    synchronize((op, case.label))
    got = device.results((op, case.label, "device"))
    if case.post is not None:
        case.post(inputs, got)
    bounds = case.bounds(inputs) if case.bounds is not None else {}
    for nsname, ns in stand_ins:
        host = SP.Side(ns, "cpu")
        case.run(host, inputs)
        want = host.results((op, case.label, nsname))
        if case.post is not None:
            case.post(inputs, want)
        assert set(bounds) <= set(want), (op, case.label, sorted(bounds), sorted(want))
        for name, ratio in SP.compare((op, case.label, nsname), got, want, bounds).items():
            print("PARITY-BOUND %s %s %s %s: error / bound = %.3g" % (op, case.label, nsname, name, ratio))


def test_fused_cases_run_on_at_least_half_of_their_shapes():
    """A fused case skips only where the real predicate refuses its shape, and no more than half of them may."""
    fused = [(op, c) for op, c in PARAMETERS if op.startswith("stencil_")]
    refused = []
    for op, case in fused:
        try:
            case.run(SP.Side(ops, DEV), case.inputs())
        except SP.Refused as why:
            refused.append((op, case.label, str(why)))
    synchronize("the fused cases")
    print("fused cases: %d, refused by the real predicate: %d" % (len(fused), len(refused)))
    for r in refused:
        print("   ", *r)
    assert len(fused) == 20 and 2 * len(refused) <= len(fused), refused


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_csr_gs_rows_against_the_oracle(order):
    """lmg_csr_gs_rows on a forward and a reversed row list of the 33 x 33 operator, bit for bit.  The rows of one call must
    be mutually independent, so the list is the 65 anti-diagonals of the grid (the five-point operator couples a node only
    to the two diagonals next to its own), one call each, 1 to 33 rows; the oracle takes the same list row by row.  b and the
    rows are left alone, nothing is written behind x."""
    A = SP.matrix("33")
    n = A.shape[0]
    x0, b = SP._vectors("gs_rows", n, n)
    y, xg = np.divmod(np.arange(n), 33)
    rows = np.argsort(xg + y, kind="stable").astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(xg + y))])
    if order == "reversed":
        rows, ptr = rows[::-1].copy(), n - ptr[::-1]
    assert ptr.size == 66 and np.diff(ptr).max() == 33 and A[rows[ptr[5]:ptr[6]]][:, rows[ptr[5]:ptr[6]]].nnz == ptr[6] - ptr[5]
    side = SP.Side(ops, DEV)
    dA, x, db, drows = side.csr("A", A), side.rw("x", x0), side.ro("b", b), side.ro("rows", rows)
    for s in range(65):
        ops.csr_gs_rows(dA, x, db, drows[ptr[s]:ptr[s + 1]])
    synchronize("csr_gs_rows")
    got = side.results(("csr_gs_rows", order))["x"]
    want = K.gs_rows(A, x0.copy(), b, rows)
    assert SP.same_bits(got, want).all(), np.flatnonzero(got != want)[:8]
    assert not np.array_equal(want, x0)
