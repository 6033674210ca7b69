"""Krylov iterations written against an ops module: restarted flexible GMRES (fgmres) and, on blocks of right-hand sides,
multigrid-preconditioned conjugate gradients with per-column scalars that stay on the device (block_pcg, block_pcg_columns).

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
    n, k = X.shape
    if k not in tuple(ops_mod.BLOCK_WIDTHS) or B.shape != X.shape or not 1 <= ncols <= k:
        raise ValueError("block_pcg: blocks %s / %s with %r columns in use" % (tuple(B.shape), tuple(X.shape), ncols))
    if bc is not None and (bc.k != k or bc.levels[0].n != n):
        raise ValueError("block_pcg: the preconditioner works on (%d, %d) blocks, not (%d, %d)" % (bc.levels[0].n, bc.k, n, k))
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


def block_pcg_columns(ops_mod, A, block_cycle, B, X0, device, *, max_iterations, error, steps=2, omega=0.8, shape="V",
                      use_graph=False):
    """block_pcg on the m >= 1 columns of the NumPy array B (n, m) from X0 (None: zero), in chunks of the widest block,
    each padded with zero columns to the narrowest width that holds it (block.block_width).  block_cycle(mc) returns the
    BlockCycle that preconditions a chunk of mc columns, ready for them (use_columns), or None: no preconditioner.
    Returns (X, track, iterations) as NumPy arrays: track has one row more than the longest chunk ran iterations, NaN
    where a column did not get that far."""
    widths = tuple(ops_mod.BLOCK_WIDTHS)
    n, m = B.shape
    X = np.empty((n, m))
    tracks, its = [], np.zeros(m, dtype=np.int64)
    for c0 in range(0, m, widths[-1]):
        mc = min(widths[-1], m - c0)
        k = block_width(mc, widths)
        bc = block_cycle(mc)
        Bk, Xk = (torch.zeros((n, k), dtype=F64, device=device) for _ in range(2))
        Bk[:, :mc].copy_(torch.from_numpy(np.ascontiguousarray(B[:, c0:c0 + mc])).to(device))
        if X0 is not None:
            Xk[:, :mc].copy_(torch.from_numpy(np.ascontiguousarray(X0[:, c0:c0 + mc])).to(device))
        rows, it_c = block_pcg(ops_mod, A, bc, Bk, Xk, ncols=mc, max_iterations=max_iterations, error=error, steps=steps,
                               omega=omega, shape=shape, use_graph=use_graph and bc is not None)
        Xh = Xk.cpu().numpy()
        if Xh[:, mc:].any():
            raise RuntimeError("a padding column of the block left zero")
        X[:, c0:c0 + mc] = Xh[:, :mc]
        its[c0:c0 + mc] = it_c
        tracks.append(np.array(rows, dtype=float).reshape(len(rows), mc))
    track = np.full((max(t.shape[0] for t in tracks), m), np.nan)
    for i, t in enumerate(tracks):
        track[:t.shape[0], i * widths[-1]:i * widths[-1] + t.shape[1]] = t
    return X, track, its


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
        g = [beta]
        cs, sn, R = [], [], []
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
            for i in range(j):                                           # the rotations of the earlier steps
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
            R.append(h)
            est = abs(g[j + 1])
            track.append(est)
            if est <= error or hn == 0.0:
                break
            ops_mod.axpby(1.0 / hn, w, 0.0, w)
        y = [0.0] * k                                                    # R y = g[:k], R[c][r] = entry (r, c)
        for i in range(k - 1, -1, -1):
            t = g[i]
            for c in range(i + 1, k):
                t -= R[c][i] * y[c]
            y[i] = t / R[i][i] if R[i][i] != 0.0 else 0.0
        ybuf[:k].copy_(torch.tensor(y, dtype=F64))
        ops_mod.multi_axpy(Z, k, ybuf, x, subtract=False)
        ops_mod.csr_residual_norm2(A, x, b, v0, part, s)
        beta = math.sqrt(s.item())
        track[-1] = beta
    if residual_out is not None:
        ops_mod.copy(v0, residual_out)
    return track, its
