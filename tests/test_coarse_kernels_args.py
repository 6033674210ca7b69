"""NULL-pointer checks of the coarse-solver entry points, through ctypes and WITHOUT a device: where no device is visible a
check that wrongly lets a call through ends in a launch error (LMG_ERR_LAUNCH), not in a kernel that reads address 0.
Skipped where a device is visible; tests/test_coarse_kernels_gpu.py holds the checks that are safe to run there."""
import ctypes

import numpy as np
import pytest

from learnmultigrid_amd import _lib

OK, ERR_ARG, ERR_LAUNCH = 0, -1, -3


@pytest.fixture(scope="module")
def L():
    _lib.build()
    lib = _lib.lib()
    if lib.lmg_device_count() > 0:
        pytest.skip("a device is visible: NULL pointers are not handed to entry points that could launch on it")
    return lib


def p(a):
    return a.ctypes.data


def test_coarse_front_refuses_a_tail_without_its_operands(L):
    """ntail > 0 reads b[perm[n + i]] whether or not there are blocks."""
    M, b, y, tail = np.ones(4), np.ones(8), np.zeros(8), np.zeros(8)
    perm = np.arange(8, dtype=np.int32)
    for nblocks, bs in ((0, 2), (1, 0), (1, 2)):
        assert L.lmg_coarse_front(nblocks, bs, p(M), None, p(perm), p(y), 4, p(tail), None) == ERR_ARG
        assert L.lmg_coarse_front(nblocks, bs, p(M), p(b), None, p(y), 4, p(tail), None) == ERR_ARG
        assert L.lmg_coarse_front(nblocks, bs, p(M), p(b), p(perm), p(y), 4, None, None) == ERR_ARG
        assert L.lmg_coarse_front(nblocks, bs, p(M), p(b), p(perm), p(y), 4, p(tail), None) == ERR_LAUNCH     # (checks passed)
    assert L.lmg_coarse_front(1, 2, None, p(b), p(perm), p(y), 0, None, None) == ERR_ARG
    assert L.lmg_coarse_front(1, 2, p(M), p(b), p(perm), None, 0, None, None) == ERR_ARG
    assert L.lmg_coarse_front(0, 2, None, None, None, p(y), 0, None, None) == OK                               # nothing to do
    assert not tail.any()


def test_csr_to_dense_refuses_missing_arrays(L):
    """rowptr lives on the device, so rowptr[n] > 0 cannot be excluded on the host: with rows, every array is needed."""
    rowptr, colidx, vals, dense = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32), np.ones(4), np.zeros(9)
    assert L.lmg_csr_to_dense(3, 3, p(rowptr), None, p(vals), p(dense), None) == ERR_ARG
    assert L.lmg_csr_to_dense(3, 3, p(rowptr), p(colidx), None, p(dense), None) == ERR_ARG
    assert L.lmg_csr_to_dense(3, 3, None, p(colidx), p(vals), p(dense), None) == ERR_ARG
    assert L.lmg_csr_to_dense(3, 3, p(rowptr), p(colidx), p(vals), None, None) == ERR_ARG
    assert L.lmg_csr_to_dense(3, 3, p(rowptr), p(colidx), p(vals), p(dense), None) == ERR_LAUNCH              # (checks passed)
    assert L.lmg_csr_to_dense(0, 3, None, None, None, None, None) == OK
    assert not dense.any()
