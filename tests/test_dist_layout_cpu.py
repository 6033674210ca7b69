"""What the distributed setup builds, checked directly (tests/test_dist_cpu.py pins it only through
bit-identical iterates): the local operators row by row against the replicated ones, the recorded
value sources, the ghost sets, the exchange plan against the vector layout and the all-gather index.
gloo on CPU with the test-only ops shim; the three cases are the smallest that reach every branch
of the setup."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from support import free_port


def _csr(M):
    return M.rowptr.numpy().astype(np.int64), M.colidx.numpy().astype(np.int64), M.vals.numpy()


def _compare_rows(local, row_ids, col_ids, replicated, must_be_real):
    """Rows of `local` against the rows `row_ids` of `replicated`: same columns (local ones mapped back
    through `col_ids`; None: already global) and same values, in storage order.  Rows flagged in
    `must_be_real` have to match, the others may be empty instead.
    Returns (number of mismatching rows, number of empty rows, number of matching non-empty rows among the others)."""
    rp, ci, va = _csr(local)
    frp, fci, fva = _csr(replicated)
    assert rp.size == row_ids.size + 1
    if col_ids is not None:
        ci = col_ids[ci]
    bad = empty = real = 0
    for i, g in enumerate(row_ids):
        s, e, fs, fe = rp[i], rp[i + 1], frp[g], frp[g + 1]
        if not must_be_real[i] and s == e:
            empty += 1
        elif np.array_equal(ci[s:e], fci[fs:fe]) and np.array_equal(va[s:e], fva[fs:fe]):
            real += 0 if must_be_real[i] else 1
        else:
            bad += 1
    return bad, empty, real


def _worker(rank, world, port, m, levels, replicate_below, halo_depth, transfer, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import cpu_ops_shim as shim
        from learnmultigrid_amd import problems as P
        from learnmultigrid_amd.dist import DistributedVCycle, _take
        A, _rhs = P.poisson_2d_structured(m)
        if transfer == "geometric":
            hier = P.geometric_hierarchy_2d(m + 1, levels)
        else:                                      # the learned-like 5 x 5 transfers of test_dist_cpu._worker
            import scipy.sparse as sp
            hier = []
            for li, sz in enumerate(P.level_sizes(m + 1, levels)[:-1]):
                l2 = P.pseudo_l2_interpolator_1d(sz)
                hier.append(P.learned_like(sp.kron(l2, l2).tocsr(), 43 + li))
        D = DistributedVCycle.from_problem(A, hier, "cpu", ops_mod=shim, grid_side=m + 1,
                                           replicate_below=replicate_below, halo_depth=halo_depth)
        fails = []

        def check(ok, *what):
            if not ok:
                fails.append(what)

        for l, d in enumerate(D.dl):
            lev = D.full.levels[l]
            lo, hi = D.bounds[l][rank], D.bounds[l][rank + 1]
            glo, ghi, rows = d.ghost_lo.numpy(), d.ghost_hi.numpy(), d.rows_global.numpy()
            owned = np.zeros(d.n_tot, dtype=bool)
            owned[d.own] = True
            ghost_rows = d.n_lo + d.n_hi
            # 6. ghost sets: sorted, outside [lo, hi), below lo / at or above hi
            check((d.lo, d.hi, d.n_own, d.n_lo, d.n_hi, d.n_tot)
                  == (lo, hi, hi - lo, glo.size, ghi.size, glo.size + hi - lo + ghi.size), l, "counts")
            check(np.all(np.diff(glo) > 0) and np.all(np.diff(ghi) > 0), l, "ghosts sorted")
            check(np.all(glo >= 0) and np.all(glo < lo) and np.all(ghi >= hi) and np.all(ghi < lev.n), l, "ghost ranges")
            check(np.array_equal(rows, np.concatenate([glo, np.arange(lo, hi), ghi])), l, "rows_global")
            # 1., 2. rows of A: owned ones equal the global rows, ghost ones are empty or equal them
            check(d.A.shape == (d.n_tot, d.n_tot), l, "A shape")
            bad, empty, real = _compare_rows(d.A, rows, rows, lev.A, owned)
            check(bad == 0 and empty + real == ghost_rows, l, "A rows", bad, empty, real)
            check(real == 0 if halo_depth == 1 else real > 0, l, "A ghost rows carrying real rows", real)
            # 3. rows of P, columns in the layout of the next level (global when that one is replicated)
            if l + 1 < D.n_dist:
                nxt = D.dl[l + 1]
                p_cols, p_ncols = nxt.rows_global.numpy(), nxt.n_tot
                r_rows, r_owned = p_cols, np.zeros(nxt.n_tot, dtype=bool)
                r_owned[nxt.own] = True
            else:
                p_cols, p_ncols = None, D.full.levels[l + 1].n
                r_rows = np.arange(D.bounds[l + 1][rank], D.bounds[l + 1][rank + 1])
                r_owned = np.ones(r_rows.size, dtype=bool)
            check(d.P.shape == (d.n_tot, p_ncols), l, "P shape")
            bad, empty, real = _compare_rows(d.P, rows, p_cols, lev.P, owned)
            check(bad == 0 and empty + real == ghost_rows, l, "P rows", bad, empty, real)
            check(real == 0 if halo_depth == 1 else real > 0, l, "P ghost rows carrying real rows", real)
            # (A and P carry real rows on the same ghost rows: the correction is applied wherever the sweeps are exact)
            check(np.array_equal(np.diff(_csr(d.A)[0]) > 0, np.diff(_csr(d.P)[0]) > 0), l, "real rows of A and of P")
            # 4. rows of R: those of the owned coarse rows equal the global rows (its ghost rows are empty)
            check(d.R.shape == (r_rows.size, d.n_tot), l, "R shape")
            bad, empty, real = _compare_rows(d.R, r_rows, rows, lev.R, r_owned)
            check(bad == 0 and real == 0 and empty == r_rows.size - int(r_owned.sum()), l, "R rows", bad, empty, real)
            # 5. value sources: what rebuild_numeric copies is what the local operator holds
            for name, local, replicated, src in (("A", d.A, lev.A, d.A_src), ("P", d.P, lev.P, d.P_src),
                                                 ("R", d.R, lev.R, d.R_src)):
                check(np.array_equal(_take(replicated.vals, src).numpy(), local.vals.numpy()), l, name + " sources")
            # 7. the exchange plan against the layout: receives tile the ghost slots, sends read owned slots only
            hits = np.zeros(d.n_tot, dtype=np.int64)
            for _q, off, cnt in d.recv:
                check(cnt > 0 and 0 <= off and off + cnt <= d.n_tot, l, "recv segment", off, cnt)
                hits[off:off + cnt] += 1
            check(np.array_equal(hits, (~owned).astype(np.int64)), l, "recv segments tile the ghost slots")
            for q, idx, _buf in d.send:
                slots = np.arange(idx[0], idx[1]) if isinstance(idx, tuple) else idx.numpy()
                check(q != rank and slots.size > 0 and np.all(owned[slots]), l, "send entry", q)
        # 8. the all-gather index puts the ranks' owned rows of the first replicated level in global order
        cb = D.bounds[D.n_dist]
        n_coarse = D.full.levels[D.n_dist].n
        check(D.ag_rows == cb[rank + 1] - cb[rank] and D.ag_max == max(np.diff(cb)), "all-gather sizes")
        D.ag_send.fill_(-1.0)
        D.ag_send[:D.ag_rows] = torch.arange(cb[rank], cb[rank + 1], dtype=torch.float64)
        dist.all_gather_into_tensor(D.ag_recv, D.ag_send)
        out = torch.full((n_coarse,), -2.0, dtype=torch.float64)
        shim.gather(D.ag_index, D.ag_recv, out)
        check(np.array_equal(out.numpy(), np.arange(n_coarse, dtype=np.float64)), "all-gather index")
        info = {"fails": fails, "n_dist": D.n_dist, "r_need": D.r_need,
                "neighbours": sorted({q for q, _o, _c in D.dl[0].recv}),
                "index_sends": sum(1 for d in D.dl for _q, idx, _b in d.send if not isinstance(idx, tuple))}
        np.save(os.path.join(out_dir, "layout_%d.npy" % rank), np.array([repr(info)]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,m,levels,replicate_below,halo_depth,transfer",
                         [(2, 32, 4, 200, 6, "geometric"),     # two distributed levels: both operator branches
                          (3, 40, 4, 300, 1, "geometric"),     # one-layer halo (no real ghost rows), an interior rank
                          (2, 48, 3, 1, 8, "learned")])        # wide rows, r_need >= 3, non-contiguous send lists
def test_local_operators_and_plans_match_the_replicated_hierarchy(tmp_path, world, m, levels, replicate_below, halo_depth,
                                                                  transfer):
    mp.spawn(_worker, args=(world, free_port(), m, levels, replicate_below, halo_depth, transfer, str(tmp_path)),
             nprocs=world, join=True)
    infos = [eval(str(np.load(os.path.join(str(tmp_path), "layout_%d.npy" % r))[0])) for r in range(world)]
    for r, info in enumerate(infos):
        assert info["fails"] == [], (r, info)
    # the cases reach what they are there for
    if transfer == "learned":
        assert all(info["n_dist"] == 2 and info["r_need"][0] >= 3 for info in infos), infos
        assert any(info["index_sends"] > 0 for info in infos), infos
    elif world == 2:
        assert all(info["n_dist"] == 2 for info in infos), infos
    else:
        assert infos[1]["neighbours"] == [0, 2], infos
