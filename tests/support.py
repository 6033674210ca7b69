"""TEST-ONLY helpers that several test modules share: moving arrays to the device and back (DEV, dev, nan_vec, to_numpy,
to_scipy), the grid operators the fused-pass and coarse-solver tests run on (galerkin_operator, galerkin9, operators), and
three small things more than one module needs: a free rendezvous port for spawned process groups (free_port), the functions
include/lmg.h declares (header_symbols), and the recorded model of golden fixture g7 (ReplayModel).  Importing it needs
neither torch, nor the package, nor a GPU: torch and learnmultigrid_amd are imported inside the functions that need them."""
import os
import re

import numpy as np
import scipy.sparse as sp

from oracle import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def dev(a, dtype=None):
    """The array as a contiguous tensor on DEV, converted to `dtype` on the host first where one is given."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def nan_vec(n):
    """An fp64 vector of NaNs on DEV: an output buffer in which every element a kernel leaves unwritten shows."""
    import torch
    return torch.full((n,), np.nan, dtype=torch.float64, device=DEV)


def to_numpy(t):
    """A CPU tensor as the NumPy array that shares its memory (writes go through)."""
    return t.numpy()


def to_scipy(A):
    """A DeviceCSR on CPU tensors as a SciPy CSR matrix on the same arrays, in storage order."""
    return sp.csr_matrix((to_numpy(A.vals), to_numpy(A.colidx), to_numpy(A.rowptr)), shape=A.shape)


def galerkin_operator(m, coarsenings=1):
    """The 9-point Galerkin operator P^T A P on the (m + 1)^2 grid, `coarsenings` tensor-product coarsenings below the
    5-point operator, with sorted rows and the index arrays as SciPy's product leaves them."""
    from learnmultigrid_amd import problems as P
    A, _ = P.poisson_2d_structured(m * 2 ** coarsenings)
    side = m * 2 ** coarsenings + 1
    for _ in range(coarsenings):
        Pm = P.tensor_interpolator_2d(side)
        A = sp.csr_matrix(Pm.T @ A @ Pm)
        side = (side - 1) // 2 + 1
    A.sort_indices()
    return A


def galerkin9(side):
    """galerkin_operator on a side^2 grid (side odd) as K.as_csr hands it on: int32 indices, float64 values."""
    return K.as_csr(galerkin_operator(side - 1))


def operators(side, kind):
    """(A, P, R) on a side^2 grid (side odd): the 5-point Poisson operator ("5pt") or the 9-point Galerkin operator of the
    next finer grid, the tensor-product interpolation onto it from ((side + 1) / 2)^2 nodes and its transpose."""
    from learnmultigrid_amd import problems as P
    A = K.as_csr(P.poisson_2d_structured(side - 1)[0]) if kind == "5pt" else galerkin9(side)
    Pm = sp.csr_matrix(P.tensor_interpolator_2d(side))
    return A, K.as_csr(Pm), K.as_csr(sp.csr_matrix(Pm.T))


def free_port():
    """A TCP port that is free now, for the rendezvous of a process group a test spawns."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def header_symbols():
    """The names of the functions include/lmg.h declares, sorted."""
    txt = open(os.path.join(ROOT, "include", "lmg.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lmg_[a-z0-9_]+)\s*\(", txt)))


class ReplayModel:
    """Feeds back the predictions recorded from the reference run (fixture g7), keyed by the
    number of patches, and checks that it is shown the same features."""

    def __init__(self, g):
        self.table = {g["features_l0"].shape[0]: (g["features_l0"], g["pred_l0"]),
                      g["features_l1"].shape[0]: (g["features_l1"], g["pred_l1"])}
        self.calls = 0

    def predict(self, data):
        feats, pred = self.table[data.shape[0]]
        np.testing.assert_allclose(data, feats, rtol=1e-11, atol=1e-16)
        self.calls += 1
        return pred
