"""Krylov iterations written against an ops module: restarted flexible GMRES (fgmres) and, on blocks of right-hand sides,
multigrid-preconditioned conjugate gradients with per-column scalars that stay on the device (block_pcg, block_pcg_columns)
and flexible GMRES with a per-column Arnoldi recurrence on the host (block_fgmres, block_fgmres_columns).

Restarted flexible GMRES, right-preconditioned: FGMRES(m) of Saad, with the Gram-Schmidt passes fused on the device.

Written against an ops module, the way Hierarchy is, so that the host logic also runs on CPU tensors under a test shim;
every vector operation is a kernel of that module (csr_spmv, csr_residual_norm2, multi_dot, multi_axpy, axpby, copy).

One cycle from the iterate x with r = b - A x, beta = |r|, v_0 = r / beta.  Step j:
    z_j = M(v_j),  w = A z_j                         (M may change from step to step: the z_j are kept, not recomputed)
    CGS2: h1 = V_j^T w, w -= V_j h1, h2 = V_j^T w, w -= V_j h2 with |w|^2 folded into the last pass -- four launches
          pairs whose coefficients never leave the device; ONE device-to-host read per step, of h1, h2 and |w|^2
    h = h1 + h2,  h_(j+1,j) = |w|,  v_(j+1) = w / h_(j+1,j)
    Givens rotations on the host keep the Hessenberg matrix triangular; |g_(j+1)| is the residual norm of the step
At the end of the cycle x += Z_k y (one multi_axpy, y uploaded) and the true residual is recomputed: it ends the
iteration or starts the next cycle.  Memory: (2 m + 1) basis vectors besides x, b and the caller's."""
import math

import numpy as np
import torch

from .block import block_width

F64 = torch.float64


class Arnoldi:
    """The least-squares problem of one column in one restart cycle, on the host: the Givens rotations (cs, sn) that keep
    the Hessenberg matrix triangular (R, column by column: R[c][r] = entry (r, c)) and the rotated right-hand side g, which
    starts as [beta]."""

    def __init__(self, beta):
        self.cs, self.sn, self.R, self.g = [], [], [], [beta]

    def step(self, h, hn):
        """Step j = len(R): h holds the j + 1 sums h1[i] + h2[i] of CGS2, hn = |w|.  Returns the estimate |g_(j+1)|."""
        cs, sn, g = self.cs, self.sn, self.g
        j = len(self.R)
        for i in range(j):                                               # the rotations of the earlier steps
            t = cs[i] * h[i] + sn[i] * h[i + 1]
            h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1]
            h[i] = t
        d = math.hypot(h[j], hn)
        c, sj = (1.0, 0.0) if d == 0.0 else (h[j] / d, hn / d)
        h[j] = c * h[j] + sj * hn
        cs.append(c)
        sn.append(sj)
        g.append(-sj * g[j])
        g[j] = c * g[j]
        self.R.append(h)
        return abs(g[j + 1])

    def solution(self):
        """y of R y = g[:k] for the k steps taken; a zero pivot gives y[i] = 0.0."""
        R, k = self.R, len(self.R)
        y = [0.0] * k
        for i in range(k - 1, -1, -1):
            t = self.g[i]
            for c in range(i + 1, k):
                t -= R[c][i] * y[c]
            y[i] = t / R[i][i] if R[i][i] != 0.0 else 0.0
        return y


def _check_blocks(name, ops_mod, bc, B, X, ncols):
    """(n, k) of the blocks of block_pcg / block_fgmres, which the width, B, ncols and the BlockCycle must fit (ValueError)."""
    n, k = X.shape
    if k not in tuple(ops_mod.BLOCK_WIDTHS) or B.shape != X.shape or not 1 <= ncols <= k:
        raise ValueError("%s: blocks %s / %s with %r columns in use" % (name, tuple(B.shape), tuple(X.shape), ncols))
    if bc is not None and (bc.k != k or bc.levels[0].n != n):
        raise ValueError("%s: the preconditioner works on (%d, %d) blocks, not (%d, %d)" % (name, bc.levels[0].n, bc.k, n, k))
    return n, k


def block_pcg(ops_mod, A, bc, B, X, *, ncols, max_iterations, error, steps=2, omega=0.8, shape="V", use_graph=False):
    """Preconditioned conjugate gradients on the columns 0 .. ncols-1 of the (n, k) blocks B and X, k in
    ops_mod.BLOCK_WIDTHS: A X = B from the iterate in X, which is updated in place.  A is the fine operator's block twin
    (ops_mod.block_twin); bc is a block.BlockCycle of the same width whose cycle(steps, omega, shape) from a zero guess is the
    preconditioner (a symmetric operator for shape "V" and "W"), or None: plain CG, Z = R and r.z = |r|^2.

    Every column runs its own recurrence: alpha_j, beta_j and the convergence test live in per-column device scalars
    (block_cg_step, block_cg_direction), so column j does what CG would do on it alone.  A column is frozen by a mask on
    the device once its recurrence norm sqrt(rr_j) is <= error: its x, r and p are not stored after that, so its solution
    is the iterate of the iteration at which it passed.  Padding columns (ncols .. k-1) and columns that start at or below
    error are frozen from the beginning.  The mask the device keeps is the only test: the host reads it back, together with
    rr, in ONE transfer of 2 k doubles per iteration and never repeats the comparison.  Everything is allocated before the
    first iteration.

    Returns (track, iterations): track is a list of rows of ncols floats -- row 0 the true ||b_j - A x_j||, then per
    iteration sqrt(rr_j), NaN for a column that was frozen before that iteration; iterations[j] counts the iterations
    column j took part in.  The loop ends when every column is frozen or after max_iterations."""
    n, k = _check_blocks("block_pcg", ops_mod, bc, B, X, ncols)
    dev = X.device
    R, P, AP = (torch.zeros((n, k), dtype=F64, device=dev) for _ in range(3))
    part = torch.empty(max(ops_mod.block_partials_count(n, k), ops_mod.block_dot_partials_count(n, k)), dtype=F64, device=dev)
    sc = torch.zeros(6 * k, dtype=F64, device=dev)                       # rr | mask | tol2 | pAp | r.z | r.z of the step before
    rr, mask, tol2, pAp, rz, rz_next = (sc[i * k:(i + 1) * k] for i in range(6))

    def precondition():
        """Z = M R and rz_next = R . Z; without a preconditioner Z is R and R . Z the rr just computed."""
        if bc is None:
            ops_mod.copy(rr, rz_next)
            return R
        Z = bc.apply(R, None, steps, omega, shape, use_graph=use_graph)
        ops_mod.block_dot(R, Z, part, rz_next)
        return Z

    ops_mod.block_residual_norm2(A, X, B, R, part, rr)
    rr0 = rr.tolist()
    track = [[math.sqrt(max(v, 0.0)) for v in rr0[:ncols]]]
    its = [0] * ncols
    t2 = float(error) * float(error)
    on = [j < ncols and rr0[j] > t2 for j in range(k)]                   # the device's test, for the start
    sc[k:3 * k].copy_(torch.tensor([1.0 if o else 0.0 for o in on] + [t2] * k, dtype=F64))
    if not any(on) or max_iterations < 1:
        return track, its
    Z = precondition()
    ops_mod.copy(Z.view(-1), P.view(-1))
    rz, rz_next = rz_next, rz
    nan = float("nan")
    for it in range(int(max_iterations)):
        ops_mod.block_spmv(A, P, AP, 1.0, 0.0)
        ops_mod.block_dot(P, AP, part, pAp)
        ops_mod.block_cg_step(rz, pAp, tol2, mask, P, AP, X, R, part, rr)
        host = sc[:2 * k].tolist()                                       # the one device-to-host read of the iteration
        track.append([math.sqrt(max(host[j], 0.0)) if on[j] else nan for j in range(ncols)])
        for j in range(ncols):
            its[j] += on[j]
        on = [v != 0.0 for v in host[k:]]
        if not any(on) or it + 1 == max_iterations:
            break
        Z = precondition()
        ops_mod.block_cg_direction(rz_next, rz, mask, Z, P)
        rz, rz_next = rz_next, rz
    return track, its


def columns_in_chunks(ops_mod, block_cycle, B, X0, device, solve_chunk, in_cycle=False):
    """The m >= 1 columns of the NumPy array B (n, m) from X0 (None: zero) in chunks of the widest block, each padded with
    zero columns to the narrowest width that holds it (block.block_width).  block_cycle(mc) returns the BlockCycle that
    preconditions a chunk of mc columns, ready for them (use_columns), or None: no preconditioner.  solve_chunk(bc, Bk, Xk, mc)
    solves the chunk in the (n, k) blocks Bk, Xk and returns (rows, iterations): rows of mc floats, mc iteration counts.
    in_cycle: Bk and Xk are the cycle's own fine blocks, which use_columns has cleared (nothing is allocated here), and the
    solution is its levels[0].x after the solve, whichever of the two iterate buffers that is by then.
    Returns (X, track, iterations) as NumPy arrays: track has as many rows as the longest chunk returned, NaN where a chunk
    returned fewer.  A padding column that is not zero afterwards is an error."""
    widths = tuple(ops_mod.BLOCK_WIDTHS)
    n, m = B.shape
    X = np.empty((n, m))
    tracks, its = [], np.zeros(m, dtype=np.int64)
    for c0 in range(0, m, widths[-1]):
        mc = min(widths[-1], m - c0)
        bc = block_cycle(mc)
        if in_cycle:
            Bk, Xk = bc.levels[0].b, bc.levels[0].x
        else:
            Bk, Xk = (torch.zeros((n, block_width(mc, widths)), dtype=F64, device=device) for _ in range(2))
        Bk[:, :mc].copy_(torch.from_numpy(np.ascontiguousarray(B[:, c0:c0 + mc])).to(device))
        if X0 is not None:
            Xk[:, :mc].copy_(torch.from_numpy(np.ascontiguousarray(X0[:, c0:c0 + mc])).to(device))
        rows, it_c = solve_chunk(bc, Bk, Xk, mc)
        Xh = (bc.levels[0].x if in_cycle else Xk).cpu().numpy()
        if Xh[:, mc:].any():
            raise RuntimeError("a padding column of the block left zero")
        X[:, c0:c0 + mc] = Xh[:, :mc]
        its[c0:c0 + mc] = it_c
        tracks.append(np.array(rows, dtype=float).reshape(len(rows), mc))
    track = np.full((max(t.shape[0] for t in tracks), m), np.nan)
    for i, t in enumerate(tracks):
        track[:t.shape[0], i * widths[-1]:i * widths[-1] + t.shape[1]] = t
    return X, track, its


def block_pcg_columns(ops_mod, A, block_cycle, B, X0, device, *, max_iterations, error, steps=2, omega=0.8, shape="V",
                      use_graph=False):
    """block_pcg on the m >= 1 columns of the NumPy array B (n, m) from X0 (None: zero), in chunks of the widest block,
    each padded with zero columns to the narrowest width that holds it (columns_in_chunks).  block_cycle(mc) returns the
    BlockCycle that preconditions a chunk of mc columns, ready for them (use_columns), or None: no preconditioner.
    Returns (X, track, iterations) as NumPy arrays: track has one row more than the longest chunk ran iterations, NaN
    where a column did not get that far."""
    def solve_chunk(bc, Bk, Xk, mc):
        return block_pcg(ops_mod, A, bc, Bk, Xk, ncols=mc, max_iterations=max_iterations, error=error, steps=steps,
                         omega=omega, shape=shape, use_graph=use_graph and bc is not None)

    return columns_in_chunks(ops_mod, block_cycle, B, X0, device, solve_chunk)


def block_fgmres(ops_mod, A, bc, B, X, *, ncols, restart, max_iterations, error, steps=2, omega=0.8, shape="V",
                 use_graph=False):
    """Right-preconditioned FGMRES(restart) on the columns 0 .. ncols-1 of the (n, k) blocks B and X, k in
    ops_mod.BLOCK_WIDTHS: A X = B from the iterate in X, which is updated in place.  A is the operator's block twin; bc is a
    block.BlockCycle of the same width whose cycle(steps, omega, shape) from a zero guess is the preconditioner M ("V", "W" or
    "F": nothing here needs a symmetric one), or None: Z is V.

    Every column runs the recurrence of fgmres on its own numbers; the block shares the matrix bytes of the cycle and of
    A Z, the launches and the host read.  Step s of a block's cycle:
        Z_s = M V_s,  W = A Z_s into V_(s+1)
        CGS2 against V_0 .. V_s as four launches (block_multi_dot, block_multi_axpy, and again with |w_j|^2 folded in);
        ONE device-to-host read of h1, h2 and the norms, (2 (restart + 1) + 1) k doubles
        per column on the host what fgmres does (one Arnoldi each): h = h1 + h2, the rotations, the estimate |g_(s+1)|
        one block_scale: 1 / |w_j| for the columns that go on, 0 for those that do not (none after the last step of a
        cycle: that block is not read again)
    A column leaves the block's cycle at its own step k_j -- its estimate is <= error, |w_j| == 0, or its own iteration
    count has reached max_iterations -- and rides through the remaining steps as zeros.  The cycle ends when no column is
    on or after `restart` steps; then X += Z y is one block_multi_axpy with k_j vectors for column j, and the true residuals
    of all columns are recomputed into V_0.  A column whose true norm is <= error, or that has used up max_iterations, is
    off for good and its X is not stored again; the others restart together.  Columns that start at or below error (or at
    zero) and the padding columns ncols .. k-1 are off from the beginning: their X keeps its bits.  Everything is
    allocated before the first step: 2 restart + 1 blocks (restart + 1 without a preconditioner).

    Returns (track, iterations): iterations[j] the inner iterations column j ran; track a list of rows of ncols floats in
    which column j is the track fgmres returns for it, written in ITS OWN iteration count -- row 0 the true initial norm, row
    i its i-th inner iteration: the Arnoldi estimate, replaced by the recomputed true norm for the last inner iteration of
    each of its cycles --, NaN behind its last iteration.  A column's history does not depend on the other columns."""
    m = int(restart)
    if m < 1:
        raise ValueError("restart must be >= 1, got %r" % (restart,))
    n, k = _check_blocks("block_fgmres", ops_mod, bc, B, X, ncols)
    dev = X.device
    V = torch.zeros((m + 1, n, k), dtype=F64, device=dev)
    Z = V if bc is None else torch.zeros((m, n, k), dtype=F64, device=dev)
    part = torch.empty(max(ops_mod.block_partials_count(n, k), ops_mod.block_multi_partials_count(n, k, m + 1)), dtype=F64,
                       device=dev)
    nh = (m + 1) * k
    hbuf = torch.zeros(2 * nh + k, dtype=F64, device=dev)                # h1 | h2 | |w_j|^2, h[i * k + j]
    h1, h2, nrm = hbuf[:nh], hbuf[nh:2 * nh], hbuf[2 * nh:]
    ybuf = torch.zeros(m * k, dtype=F64, device=dev)

    ops_mod.block_residual_norm2(A, X, B, V[0], part, nrm)
    beta = [math.sqrt(v) for v in nrm.tolist()]
    tracks = [[beta[j]] for j in range(ncols)]
    its = [0] * ncols

    def goes_on(j):
        return j < ncols and beta[j] > error and beta[j] > 0.0 and its[j] < max_iterations

    on = [goes_on(j) for j in range(k)]
    while any(on):
        ops_mod.block_scale([1.0 / beta[j] if on[j] else 0.0 for j in range(k)], V[0])
        ls = [Arnoldi(beta[j]) for j in range(k)]
        kj = [0] * k
        for s in range(m):
            W = V[s + 1]
            zs = V[s] if bc is None else bc.apply(V[s], Z[s], steps, omega, shape, use_graph=use_graph)
            ops_mod.block_spmv(A, zs, W, 1.0, 0.0)
            counts = [s + 1 if on[j] else 0 for j in range(k)]
            ops_mod.block_multi_dot(V, s + 1, W, part, h1)
            ops_mod.block_multi_axpy(V, counts, h1, W)
            ops_mod.block_multi_dot(V, s + 1, W, part, h2)
            ops_mod.block_multi_axpy(V, counts, h2, W, part, nrm)
            hb = hbuf.tolist()                                           # the one device-to-host read of the step
            scale = [0.0] * k
            for j in range(k):
                if not on[j]:
                    continue
                h = [hb[i * k + j] + hb[nh + i * k + j] for i in range(s + 1)]
                hn = math.sqrt(hb[2 * nh + j])
                its[j] += 1
                kj[j] = s + 1
                est = ls[j].step(h, hn)
                tracks[j].append(est)
                if est <= error or hn == 0.0 or its[j] == max_iterations:
                    on[j] = False                                        # leaves the cycle at k_j = s + 1
                else:
                    scale[j] = 1.0 / hn
            if not any(on) or s + 1 == m:
                break
            ops_mod.block_scale(scale, W)
        y = [0.0] * (m * k)                                              # y[i * k + j]: k_j entries for column j
        for j in range(k):
            y[j:kj[j] * k:k] = ls[j].solution()
        ybuf.copy_(torch.tensor(y, dtype=F64))
        ops_mod.block_multi_axpy(Z, kj, ybuf, X, subtract=False)
        ops_mod.block_residual_norm2(A, X, B, V[0], part, nrm)
        true = nrm.tolist()
        for j in range(k):
            if kj[j]:
                beta[j] = math.sqrt(true[j])
                tracks[j][-1] = beta[j]
        on = [goes_on(j) for j in range(k)]
    nan = float("nan")
    rows = max(len(t) for t in tracks)
    return [[t[i] if i < len(t) else nan for t in tracks] for i in range(rows)], its


def block_fgmres_columns(ops_mod, A, block_cycle, B, X0, device, *, restart, max_iterations, error, steps=2, omega=0.8,
                         shape="V", use_graph=False):
    """block_fgmres on the m >= 1 columns of the NumPy array B (n, m) from X0 (None: zero), chunked and padded like
    block_pcg_columns (columns_in_chunks, which also checks that the padding columns are still zero).  Returns
    (X, track, iterations) as NumPy arrays: column j of track is that column's own history, NaN behind its last iteration."""
    def solve_chunk(bc, Bk, Xk, mc):
        return block_fgmres(ops_mod, A, bc, Bk, Xk, ncols=mc, restart=restart, max_iterations=max_iterations, error=error,
                            steps=steps, omega=omega, shape=shape, use_graph=use_graph and bc is not None)

    return columns_in_chunks(ops_mod, block_cycle, B, X0, device, solve_chunk)


def fgmres(ops_mod, A, b, x, apply_M, *, restart, max_iterations, error, residual_out=None):
    """Solve A x = b from the iterate in x (updated in place); apply_M(src, dst) writes dst = M(src), None: identity.
    Returns (track, iterations): track[0] the true initial |b - A x|, then one entry per inner iteration -- the Arnoldi
    estimate, replaced by the recomputed true norm for the last iteration of every cycle; iterations = inner iterations =
    preconditioner applications = len(track) - 1.  Convergence is declared on a true norm <= error only.
    residual_out: receives b - A x of the returned x."""
    m = int(restart)
    if m < 1:
        raise ValueError("restart must be >= 1, got %r" % (restart,))
    n = x.numel()
    dev = x.device
    ldv = n + (n & 1)                              # even: every row of a basis starts on 16 bytes
    V = torch.empty((m + 1, ldv), dtype=F64, device=dev)
    Z = V if apply_M is None else torch.empty((m, ldv), dtype=F64, device=dev)
    part = torch.empty(max(ops_mod.partials_count(n), ops_mod.multi_partials_count(n, m + 1)), dtype=F64, device=dev)
    hbuf = torch.zeros(2 * (m + 1) + 1, dtype=F64, device=dev)           # h1 | h2 | |w|^2
    h1, h2, nrm = hbuf[:m + 1], hbuf[m + 1:2 * (m + 1)], hbuf[2 * (m + 1):]
    ybuf = torch.zeros(m, dtype=F64, device=dev)
    s = torch.zeros(1, dtype=F64, device=dev)
    v0 = V[0, :n]

    ops_mod.csr_residual_norm2(A, x, b, v0, part, s)
    beta = math.sqrt(s.item())
    track = [beta]
    its = 0
    while beta > error and beta > 0.0 and its < max_iterations:
        ops_mod.axpby(1.0 / beta, v0, 0.0, v0)
        ls = Arnoldi(beta)
        k = 0
        for j in range(m):
            if its == max_iterations:
                break
            vj, w = V[j, :n], V[j + 1, :n]
            zj = vj
            if apply_M is not None:
                zj = Z[j, :n]
                apply_M(vj, zj)
            ops_mod.csr_spmv(A, zj, w, 1.0, 0.0)
            ops_mod.multi_dot(V, j + 1, w, part, h1)
            ops_mod.multi_axpy(V, j + 1, h1, w)
            ops_mod.multi_dot(V, j + 1, w, part, h2)
            ops_mod.multi_axpy(V, j + 1, h2, w, part, nrm)
            hb = hbuf.tolist()                                           # the one device-to-host read of the step
            h = [hb[i] + hb[m + 1 + i] for i in range(j + 1)]
            hn = math.sqrt(hb[2 * (m + 1)])
            its += 1
            k = j + 1
            est = ls.step(h, hn)
            track.append(est)
            if est <= error or hn == 0.0:
                break
            ops_mod.axpby(1.0 / hn, w, 0.0, w)
        ybuf[:k].copy_(torch.tensor(ls.solution(), dtype=F64))
        ops_mod.multi_axpy(Z, k, ybuf, x, subtract=False)
        ops_mod.csr_residual_norm2(A, x, b, v0, part, s)
        beta = math.sqrt(s.item())
        track[-1] = beta
    if residual_out is not None:
        ops_mod.copy(v0, residual_out)
    return track, its
