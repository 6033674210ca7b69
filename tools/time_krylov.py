#!/usr/bin/env python3
"""One Gram-Schmidt orthogonalisation of a vector against j + 1 basis vectors at 4097^2 unknowns, timed with device events
after a warm-up: the fused CGS2 of krylov.fgmres (multi_dot, multi_axpy, multi_dot, multi_axpy with the norm, one
device-to-host read) next to what the vector kernels alone offer (modified Gram-Schmidt: dot + .item() + axpby per basis
vector, then the norm), the two alternating in the same run.  Throughput against the model (4 (j + 1) + 4) 8 n bytes of the
fused step (each pass reads the basis once; w is read four times and written twice, rounded to 4), and the device-copy
rate of the same run as the ceiling.

    python tools/time_krylov.py [--side 4097] [--depths 5,15,30] [--reps 10] [--rounds 3]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                   # noqa: E402
from learnmultigrid_amd import ops             # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=4097)
ap.add_argument("--depths", default="5,15,30")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
depths = [int(d) for d in args.depths.split(",")]

if not torch.cuda.is_available():
    sys.exit("time_krylov.py needs the GPU: a time from anywhere else says nothing")
dev = torch.device("cuda:0")
F64 = torch.float64
n = args.side * args.side
ldv = n + (n & 1)
kmax = max(depths)
rows = max(kmax, 16)
torch.manual_seed(7)
V = torch.empty((rows, ldv), dtype=F64, device=dev)
for j in range(rows):                          # rows of norm ~ 1, nearly orthogonal: repeated passes stay bounded
    V[j].normal_(0.0, n ** -0.5)
w = torch.randn(n, dtype=F64, device=dev)
part = torch.empty(max(ops.partials_count(n), ops.multi_partials_count(n, kmax)), dtype=F64, device=dev)
hbuf = torch.zeros(2 * kmax + 1, dtype=F64, device=dev)
s = torch.zeros(1, dtype=F64, device=dev)


def fused(k):
    h1, h2, nrm = hbuf[:k], hbuf[kmax:kmax + k], hbuf[2 * kmax:]
    ops.multi_dot(V, k, w, part, h1)
    ops.multi_axpy(V, k, h1, w)
    ops.multi_dot(V, k, w, part, h2)
    ops.multi_axpy(V, k, h2, w, part, nrm)
    return hbuf.tolist()


def unfused(k):
    for j in range(k):
        vj = V[j, :n]
        ops.dot(vj, w, part, s)
        ops.axpby(-s.item(), vj, 1.0, w)
    ops.dot(w, w, part, s)
    return s.item()


def copy_rows(k):
    half = rows // 2
    ops.copy(V[:half].view(-1), V[half:2 * half].view(-1))
    return 2 * half * ldv * 8


def timed_ms(f, k, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f(k)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


saved = V[rows // 2:].clone()
copy_rows(0)
torch.cuda.synchronize()
copy_ms = min(timed_ms(copy_rows, 0, args.reps) for _ in range(args.rounds))
copy_bytes = copy_rows(0)
V[rows // 2:] = saved
del saved
torch.cuda.synchronize()
ceiling = copy_bytes / (copy_ms * 1e-3)
print("n = %d^2 = %d, device copy of %.2f GB (read + write): %.3f ms = %.2f TB/s" % (args.side, n, copy_bytes / 1e9, copy_ms,
                                                                                   ceiling / 1e12))
print("| j+1 | fused CGS2 ms (min / median) | model GB | fused TB/s | of the copy rate | dot+axpby MGS ms (min / median) | MGS / fused |")
print("|---|---|---|---|---|---|---|")
for k in depths:
    w.normal_()
    fused(k), unfused(k)                       # warm-up of every shape the window uses
    torch.cuda.synchronize()
    tf, tu = [], []
    for _ in range(args.rounds):               # alternate the two versions in the same run
        tf.append(timed_ms(fused, k, args.reps))
        tu.append(timed_ms(unfused, k, args.reps))
    model = (4 * k + 4) * 8 * n
    rate = model / (min(tf) * 1e-3)
    print("| %d | %.3f / %.3f | %.2f | %.2f | %.0f %% | %.3f / %.3f | %.2f |"
          % (k, min(tf), statistics.median(tf), model / 1e9, rate / 1e12, 100 * rate / ceiling, min(tu), statistics.median(tu),
             min(tu) / min(tf)))
