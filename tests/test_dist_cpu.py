"""Multi-rank host logic on CPU: world_size-2 (and 3) gloo runs of the row-block
partitioned V-cycle, with a TEST-ONLY ops shim standing in for the HIP kernels.

Checked: every rank's slice of the distributed iterate is BIT-identical to the
single-process iterate (Jacobi row sums keep their storage order across the partition),
the all-reduced residual norm agrees to 1e-13, partitions fall on grid lines, and the
ghost layout is what A, R and P need.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from support import free_port


def _worker(rank, world, port, m, levels, replicate_below, steps, halo_depth, out_dir, transfer="geometric"):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import cpu_ops_shim as shim
        from learnmultigrid_amd import problems as P
        from learnmultigrid_amd.dist import DistributedVCycle
        from learnmultigrid_amd.hierarchy import Hierarchy
        A, rhs = P.poisson_2d_structured(m)
        A_ref = A.copy()           # on the CPU the tensors alias the SciPy buffers: keep a pristine copy for the reference run
        if transfer == "geometric":
            hier = P.geometric_hierarchy_2d(m + 1, levels)
        else:
            # learned-like transfers with the 5 x 5 support of the L2 projections: the restriction
            # reads residuals several matrix hops away, the Galerkin operators have 25-49 entries per row
            import scipy.sparse as sp
            hier = []
            for li, sz in enumerate(P.level_sizes(m + 1, levels)[:-1]):
                l2 = P.pseudo_l2_interpolator_1d(sz)
                hier.append(P.learned_like(sp.kron(l2, l2).tocsr(), 43 + li))
        D = DistributedVCycle.from_problem(A, hier, "cpu", ops_mod=shim, grid_side=m + 1,
                                           replicate_below=replicate_below, halo_depth=halo_depth)
        D.set_rhs(rhs)
        norms = [D.residual_norm()]
        per_cycle = []
        for _ in range(3):
            before = D.n_exchanges
            D.cycle("Jacobi", steps, 0.8)
            per_cycle.append(D.n_exchanges - before)
            norms.append(D.residual_norm())
        if transfer == "learned":
            # config #5: new coefficients on the same pattern -> numeric Galerkin rebuild, then go on
            rng = np.random.default_rng(77)
            new_vals = torch.from_numpy(np.ascontiguousarray(A_ref.tocsr().data * (1.0 + 0.2 * rng.random(A.nnz))))
            D.rebuild_numeric(new_vals)
            for _ in range(2):
                D.cycle("Jacobi", steps, 0.8)
                norms.append(D.residual_norm())
        x = D.gather_solution()
        # single-process run of the same arithmetic
        H = Hierarchy(A_ref, hier, "cpu", ops_mod=shim)
        H.levels[0].b.copy_(torch.from_numpy(rhs.ravel().copy()))
        ref_norms = [H.residual_norm()]
        for _ in range(3):
            H.cycle("Jacobi", steps, 0.8)
            ref_norms.append(H.residual_norm())
        if transfer == "learned":
            H.rebuild_numeric(new_vals)
            for _ in range(2):
                H.cycle("Jacobi", steps, 0.8)
                ref_norms.append(H.residual_norm())
        xr = H.levels[0].x.numpy()
        side = m + 1
        info = {"bit_identical": bool(np.array_equal(x, xr)),
                "norm_rel": float(max(abs(a - b) / b for a, b in zip(norms, ref_norms))),
                "contracting": bool(norms[3] < (0.05 if transfer == "geometric" else 0.9) * norms[0]),
                "n_dist": D.n_dist, "exchanges_per_cycle": per_cycle, "r_need": D.r_need,
                "cuts_on_lines": all(c % sd == 0 for l, sd in enumerate(P.level_sizes(side, D.n_dist + 1))
                                     for c in D.bounds[l]),
                "ghosts": [d.n_lo + d.n_hi for d in D.dl],
                "neighbours": [sorted(q for q, _o, _c in d.recv) for d in D.dl],
                # the exchange plan of every level: (peer, number of values) of every message
                "send": [sorted((int(q), int(idx[1] - idx[0]) if isinstance(idx, tuple) else int(idx.numel())) for q, idx, _b in d.send)
                         for d in D.dl],
                "recv": [sorted((int(q), int(c)) for q, _o, c in d.recv) for d in D.dl]}
        with pytest.raises(ValueError):
            D.cycle("SOR", 1, 1.0)
        np.save(os.path.join(out_dir, "info_%d.npy" % rank), np.array([repr(info)]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,m,levels,replicate_below,steps,halo_depth",
                         [(2, 32, 4, 200, 2, 6), (2, 48, 3, 1, 2, 6), (3, 40, 4, 300, 2, 6),
                          (2, 48, 3, 1, 3, 8),          # 2 nu + 2 = halo depth: one exchange per level
                          (2, 48, 3, 1, 3, 6),          # nu + 3 = halo depth: the coarse corrections travel too
                          (2, 48, 3, 1, 3, 5),          # fine level one layer short (its restriction reads two hops away)
                          (2, 48, 3, 1, 4, 5),          # deeper cycle than the halo: exchange before every sweep
                          (3, 40, 4, 300, 2, 1),        # classic one-layer halo (empty ghost rows)
                          (4, 64, 4, 500, 3, 8),        # four ranks, V(3,3) like the bench
                          (8, 128, 4, 2000, 3, 8)])     # the bench's N = 8 topology in small: two distributed levels
def test_distributed_vcycle_matches_single_process(tmp_path, world, m, levels, replicate_below, steps, halo_depth):
    port = free_port()
    mp.spawn(_worker, args=(world, port, m, levels, replicate_below, steps, halo_depth, str(tmp_path)),
             nprocs=world, join=True)
    infos = [eval(str(np.load(os.path.join(str(tmp_path), "info_%d.npy" % r))[0])) for r in range(world)]
    # every message has its counterpart: rank r sends c values to q on level l  <=>  q expects c values from r
    for l in range(infos[0]["n_dist"]):
        sends = sorted((r, q, c) for r in range(world) for q, c in infos[r]["send"][l])
        recvs = sorted((q, r, c) for r in range(world) for q, c in infos[r]["recv"][l])
        assert sends == recvs, (l, sends, recvs)
    for r in range(world):
        info = infos[r]
        assert info["bit_identical"], info
        assert info["norm_rel"] < 1e-13, info
        assert info["contracting"], info
        assert info["cuts_on_lines"], info
        assert info["n_dist"] >= 1
        # number of halo exchanges of one cycle with the deep halo: x (b on coarse levels) before
        # pre-smoothing and the coarse correction before prolongation (none below the deepest
        # distributed level) -- 2 per level minus 1; one more per level when the halo is too thin to
        # apply the correction on the ghost layers; 2 nu + 2 (+1) with one exchange per use
        nd = info["n_dist"]
        deep = [steps + 1 + max(1, rn) <= halo_depth for rn in info["r_need"]]
        local_up = 2 * steps <= halo_depth            # the correction is applied on the ghost layers too
        if all(deep):
            # one message per level; one more per level (but the deepest) when post-smoothing leaves
            # too few exact layers for the finer level's prolongation; a third one when the halo is
            # too thin to keep the corrected iterate exact on nu layers
            lo_n, hi_n = nd, (2 if local_up else 3) * nd - 1
            assert all(lo_n <= c <= hi_n for c in info["exchanges_per_cycle"]), info
            if halo_depth >= 2 * steps + 2:
                assert all(c == nd for c in info["exchanges_per_cycle"]), info
        elif not any(deep):
            assert all(c >= (2 * steps + 1) * nd for c in info["exchanges_per_cycle"]), info
        # the 9-point restriction of a 5-point operator reads residuals two matrix hops away
        assert info["r_need"][0] == (2 if halo_depth >= 2 else 1 << 20), info
        # interior ranks talk to two neighbours, edge ranks to one (thin coarse blocks of these tiny
        # test grids may reach one rank further with the deep halo)
        want = [q for q in (r - 1, r + 1) if 0 <= q < world]
        assert all(set(want) <= set(nb) for nb in info["neighbours"]), info
        assert info["neighbours"][0] == want, info


def test_block_bounds():
    from learnmultigrid_amd.dist import block_bounds
    assert block_bounds(4097, 8) == [0, 513, 1025, 1537, 2049, 2561, 3073, 3585, 4097]
    assert block_bounds(5, 2) == [0, 3, 5]
    b = block_bounds(10, 4)
    assert b[0] == 0 and b[-1] == 10 and max(np.diff(b)) - min(np.diff(b)) <= 1


@pytest.mark.parametrize("halo_depth,steps", [(8, 2), (12, 2), (4, 2)])
def test_distributed_vcycle_with_wide_learned_transfers(tmp_path, halo_depth, steps):
    """Wide transfer operators change what the halo must cover (r_need, p_need are measured from
    the matrices): whatever the depth allows, the iterate must stay bit-identical."""
    world, m, levels, replicate_below = 2, 48, 3, 1
    port = free_port()
    mp.spawn(_worker, args=(world, port, m, levels, replicate_below, steps, halo_depth, str(tmp_path), "learned"),
             nprocs=world, join=True)
    counts = []
    for r in range(world):
        info = eval(str(np.load(os.path.join(str(tmp_path), "info_%d.npy" % r))[0]))
        assert info["bit_identical"], info
        assert info["norm_rel"] < 1e-13, info
        assert info["r_need"][0] >= 3, info                 # 25-entry restriction rows on a 5-point operator
        counts.append(info["exchanges_per_cycle"])
    assert counts[0] == counts[1]                            # both ranks took the same branches


def _gs_worker(rank, world, port, m, levels, replicate_below, halo_depth, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import cpu_ops_shim as shim
        from learnmultigrid_amd import problems as P
        from learnmultigrid_amd.dist import DistributedVCycle
        from oracle import vcycle_ref as V
        A, rhs = P.poisson_2d_structured(m)
        A_ref = A.copy()
        hier = P.geometric_hierarchy_2d(m + 1, levels)
        D = DistributedVCycle.from_problem(A, hier, "cpu", ops_mod=shim, grid_side=m + 1,
                                           replicate_below=replicate_below, halo_depth=halo_depth)
        twin = V.HybridGSVCycle(A_ref, hier, [D.bounds[l] for l in range(D.n_dist)])
        b = rhs.ravel().copy()
        # (1) one smoothing step of three block sweeps on the fine level, from a random iterate: bitwise
        rng = np.random.default_rng(3)
        x0 = rng.standard_normal(A.shape[0])
        D.set_rhs(rhs)
        D.set_x(x0)
        D._smooth_gs(D.dl[0], 3, False)
        got = D.gather_solution()
        want = twin.smooth(0, x0.copy(), b, "GaussSeidel", 3, 1.0)
        smooth_equal = bool(np.array_equal(got, want))
        # (2) whole cycles with the shipped smoother: residual history against the twin
        D.set_x(np.zeros(A.shape[0]))
        norms = [D.residual_norm()]
        x = np.zeros(A.shape[0])
        ref = [float(np.linalg.norm(b - A_ref @ x))]
        for _ in range(3):
            D.cycle("GaussSeidel", 2)
            norms.append(D.residual_norm())
            x = twin.cycle(x, b, "GaussSeidel", 2, 1.0)
            ref.append(float(np.linalg.norm(b - A_ref @ x)))
        xs = D.gather_solution()
        info = {"smooth_equal": smooth_equal, "norms": norms, "ref": ref, "n_dist": D.n_dist,
                "x_err": float(np.abs(xs - x).max() / np.abs(x).max())}
        np.save(os.path.join(out_dir, "gsinfo_%d.npy" % rank), np.array([repr(info)]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,m,levels,replicate_below,halo_depth", [(2, 32, 3, 200, 1), (3, 40, 3, 300, 1), (2, 48, 3, 1, 6)])
def test_distributed_processor_block_gauss_seidel_matches_its_cpu_twin(tmp_path, world, m, levels, replicate_below, halo_depth):
    """The shipped smoother across ranks: every rank relaxes its rows in lexicographic order with the ghost values of the
    start of the sweep.  One smoothing step is bit-identical to the CPU twin (oracle.vcycle_ref.HybridGSVCycle), whole
    V-cycles agree with it at 1e-10 (the coarsest solve is SuperLU there, explicit block inverses here); with the classic
    one-layer halo and with a deep one (owned rows only are relaxed either way)."""
    port = free_port()
    mp.spawn(_gs_worker, args=(world, port, m, levels, replicate_below, halo_depth, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        info = eval(str(np.load(os.path.join(str(tmp_path), "gsinfo_%d.npy" % r))[0]))
        assert info["smooth_equal"], info
        np.testing.assert_allclose(info["norms"], info["ref"], rtol=1e-10, atol=1e-14 * info["ref"][0])
        assert info["x_err"] < 1e-9, info
        assert info["norms"][3] < 0.05 * info["norms"][0], info          # it still is a multigrid cycle
