"""Restarted flexible GMRES, right-preconditioned: FGMRES(m) of Saad, with the Gram-Schmidt passes fused on the device.

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

import torch

F64 = torch.float64


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
