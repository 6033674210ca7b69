"""Every compiled sliced-ELL sweep (csrc/sell.hip) against the CPU oracle on the CSR matrix, bit for bit (-m gpu).

54 kernels are compiled -- 3 modes x 2 column widths x (JU 4; JU 5, 7, 8, 10 each cached and nontemporal) -- and the
launcher picks among them from the longest row and the size; pack() sends only near-uniform long rows there.  Here the
twin is built directly (SellCSR.from_csr with its overrides: int32 columns and any padding at a few hundred rows) and
hung on the operator, and sell_ju / sell_nt force every instantiation:

  uniform_L   n = 200 (three full slices and one of 8 rows), every row L entries.  13: the first length past the JU-4
              kernel; 35 = 5 * 7; 40 = 5 * 8 = 4 * 10; 41: remainder 1 for JU 5, 8, 10 and 6 for JU 7
  short_9     n = 130, 9 entries per row: the JU-4 kernel, whatever sell_ju and sell_nt say
  ragged      n = 321 (five slices and one of a single row): a slice that mixes the lengths 0 .. 30, an all-empty slice,
              a slice whose longest row has 1 entry, empty rows between long ones, rows without a diagonal entry

Outputs are the head of a longer allocation whose tail must keep its sentinel, and start as NaN wherever the kernel must
not read them (sweep_variants.check_sweeps)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sweep_variants as SV                                          # noqa: E402
from learnmultigrid_amd import ops                                   # noqa: E402
from oracle import kernels as K                                      # noqa: E402  (checker only)

DEV = SV.DEV
CASES, JUS, NTS, problem = SV.SELL_CASES, SV.SELL_JUS, SV.SELL_NTS, SV.sell_problem


def sell_operator(A, colmode):
    """The operator with a sliced-ELL twin built directly and nothing else, so that ops._sweep takes the SELL branch."""
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    S = ops.SellCSR.from_csr(dA, colmode=colmode, max_padding=float("inf"))
    assert S is not None
    dA.sell = S
    assert dA.patterns is None and dA.stencil is None and dA.packed is None and ops._PACKED_ENABLED
    lens = np.diff(A.indptr)
    n = A.shape[0]
    want_len = [int(lens[s:s + 64].max()) for s in range(0, n, 64)]
    assert S.colmode == colmode and S.max_len == int(lens.max()), (S.colmode, S.max_len)
    assert S.slice_len.cpu().tolist() == want_len and S.padded == 64 * sum(want_len)
    assert S.col.dtype == (torch.int16, torch.int32)[colmode]
    return dA, S


@pytest.mark.parametrize("colmode", [0, 1], ids=["col16", "col32"])
@pytest.mark.parametrize("name", CASES)
def test_every_sell_kernel_bit_exact(name, colmode):
    pr = problem(name)
    dA, S = sell_operator(pr.A, colmode)
    if name == "short_9":
        assert S.max_len <= 12                                   # the JU-4 kernel: the keys change nothing
    else:
        assert S.max_len > 12
    if name == "ragged_slices":
        assert S.slice_len.cpu().tolist() == [20, 30, 0, 1, 30, 17]
        assert (pr.A.diagonal() == 0.0).sum() > 64               # rows without a diagonal entry keep x
    for ju in JUS:
        for nt in NTS:
            with SV.tuned(sell_ju=ju, sell_nt=nt):
                SV.check_sweeps((name, colmode, "sell_ju", ju, "sell_nt", nt), dA, pr)


@pytest.mark.parametrize("colmode", [0, 1], ids=["col16", "col32"])
def test_new_values_on_the_same_ragged_pattern(colmode):
    """update_values rewrites the value stream only: the padding slots, the columns and the slice table stay."""
    pr = problem("ragged_slices")
    dA, S = sell_operator(pr.A, colmode)
    B = pr.A.copy()
    B.data = np.random.default_rng(7).standard_normal(B.nnz)
    dA.vals.copy_(SV.dev(B.data))
    dA.repack_values()
    assert dA.sell is S
    want = K.jacobi(B, pr.x, pr.b, 0.8)
    for ju in (7, 10):
        with SV.tuned(sell_ju=ju):
            out = SV.Guarded(B.shape[0])
            ops.csr_jacobi(dA, SV.dev(pr.x), SV.dev(pr.b), 0.8, out.out)
            got = out.result(("update_values", ju))
            assert np.array_equal(got, want), (ju, SV.first_diff(got, want))
