// Line relaxation: the tridiagonal systems of the grid lines of a level, factored once (lmg_line_factor) and solved
// per half-sweep (lmg_line_solve) by the Thomas algorithm, one lane per system.
//
// A level has n rows and a line stride W, n = H * W.  Direction x (0): system k = storage line k, element j at
// k * W + j, H systems of length W.  Direction y (1): system k = grid column k, element j at j * W + k, W systems of
// length H.  The factorisation and the per-lane solve are kernel templates over the direction.
//
// The dependent chain of a system cannot be shortened, but its loads do not depend on it, and with one lane per system a
// level offers only a few dozen waves: the solves are bound by the latency of their loads.  So every pass moves blocks of
// elements whose loads are all issued before the chain runs over them (a wave can have 64 loads in flight).  In
// direction y the 64 lanes of a wave read 64 consecutive doubles per element; in direction x every lane walks its own
// line and reads 32 bytes at a time.  (Staging 64 lines x 32 columns per array through LDS for direction x -- coalesced
// loads, a transposed read per lane, the next tile's loads in flight during the chain -- was built and measured: slower
// at 2049^2, a tie at 4097^2)
//
// The 25- and 49-point levels of learned transfers have pentadiagonal and heptadiagonal line systems: banded LU with
// half-bandwidth P = 2, 3 (lmg_line_factor_banded, lmg_line_solve_banded), the same shape -- one lane per system, blocks
// of loads issued before the chain -- in the second half of this file.  The tridiagonal pair is not touched by it.
#include "lmg_common.hpp"

namespace {

constexpr int kBlock = 256;         // the row-parallel extraction
constexpr int kLineBlock = 64;      // one wave per workgroup: the few dozen waves of a level spread over the CUs
constexpr int kFactorChunk = 8;     // elements per block of loads: the factorisation (setup) and the ends of a solve ...
constexpr int kSolveChunkY = 16;    // ... the solve in direction y: 48 coalesced 8-byte loads in flight per wave ...
constexpr int kSolveChunkX = 32;    // ... and in direction x: 48 loads of 16 bytes per lane
constexpr int kBandFactorChunk = 4;  // the banded systems: the factorisation moves 2 P + 1 planes, 28 loads per block for P = 3
constexpr int kBandShort = 8;       // ... and their solves go in blocks of kSolveChunkX / kSolveChunkY, then 8, then single elements
constexpr int kMaxGrid = 256 * 8;

enum { DIR_X = 0, DIR_Y = 1 };

struct __attribute__((aligned(8))) d4u { double v[4]; };      // 32 bytes at 8-byte alignment (a line starts anywhere)

// N elements of a system from element pointer p (stride inc between elements: 1 in direction x, W in direction y)
template <int DIR, int N>
__device__ __forceinline__ void load_chunk(const double *p, int64_t inc, double (&out)[N])
{
    if (DIR == DIR_X) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const d4u t = *reinterpret_cast<const d4u *>(p + 4 * q);
#pragma unroll
            for (int u = 0; u < 4; ++u) out[4 * q + u] = t.v[u];
        }
    } else {
#pragma unroll
        for (int u = 0; u < N; ++u) out[u] = p[u * inc];
    }
}

template <int DIR, int N>
__device__ __forceinline__ void store_chunk(double *p, int64_t inc, const double (&in)[N])
{
    if (DIR == DIR_X) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            d4u t;
#pragma unroll
            for (int u = 0; u < 4; ++u) t.v[u] = in[4 * q + u];
            *reinterpret_cast<d4u *>(p + 4 * q) = t;
        }
    } else {
#pragma unroll
        for (int u = 0; u < N; ++u) p[u * inc] = in[u];
    }
}

// The tridiagonal part of every row from the sorted CSR: lo[i], a[i], up[i] = the entries at column - row = -s, 0, +s
// (s = 1 in direction x, W in direction y; a missing entry is 0).  In direction x the sub-diagonal entry of the first row
// of a line and the super-diagonal entry of its last row belong to no system: they couple two lines, and a non-zero
// one sets bit 0 of *flags.
template <int DIR>
__global__ void __launch_bounds__(kBlock) line_extract_kernel(int64_t n, int64_t W, const int *rowptr, const int *colidx,
                                                              const double *vals, double *lo, double *a, double *up,
                                                              int *flags)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t s = DIR == DIR_X ? 1 : W;
    bool coupled = false;
    for (int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x; row < n; row += stride) {
        double l = 0.0, d = 0.0, u = 0.0;
        for (int e = rowptr[row]; e < rowptr[row + 1]; ++e) {
            const int64_t off = (int64_t)colidx[e] - row;
            const double v = vals[e];
            if (off == -s) l = v;
            else if (off == 0) d = v;
            else if (off == s) u = v;
        }
        if (DIR == DIR_X) {
            const int64_t col = row % W;
            if (col == 0) {
                coupled |= (l != 0.0);
                l = 0.0;
            }
            if (col == W - 1) {
                coupled |= (u != 0.0);
                u = 0.0;
            }
        }
        lo[row] = l;
        a[row] = d;
        up[row] = u;
    }
    if (coupled) atomicOr(flags, 1);
}

// One step of the factorisation: den = a - lo * cp_prev, minv = 1 / den, cp = up * minv.
__device__ __forceinline__ void factor_step(double lo, double a, double up, double &cp, double &minv, bool &bad)
{
    const double den = a - lo * cp;
    bad |= !(den != 0.0 && fabs(den) <= 1.79769313486231570815e+308);      // zero, infinite or NaN
    minv = 1.0 / den;
    cp = up * minv;
}

// The factorisation along every system, in place: a (in minv) -> minv, up (in cp) -> cp.  Lane <-> system.
template <int DIR>
__global__ void __launch_bounds__(kLineBlock) line_recur_kernel(int64_t nsys, int64_t L, int64_t W, const double *lo,
                                                                double *minv, double *cp, int *flags)
{
    constexpr int N = kFactorChunk;
    const int64_t k = (int64_t)blockIdx.x * kLineBlock + threadIdx.x;
    if (k >= nsys) return;
    const int64_t base = DIR == DIR_X ? k * W : k, inc = DIR == DIR_X ? 1 : W;
    bool bad = false;
    // den_0 = a_0
    const double den0 = minv[base];
    bad |= !(den0 != 0.0 && fabs(den0) <= 1.79769313486231570815e+308);
    double m = 1.0 / den0;
    double c = cp[base] * m;
    minv[base] = m;
    cp[base] = c;
    int64_t j = 1;
    for (; j + N <= L; j += N) {
        const int64_t at = base + j * inc;
        double l8[N], a8[N], u8[N];
        load_chunk<DIR, N>(lo + at, inc, l8);
        load_chunk<DIR, N>(minv + at, inc, a8);
        load_chunk<DIR, N>(cp + at, inc, u8);
#pragma unroll
        for (int u = 0; u < N; ++u) {
            factor_step(l8[u], a8[u], u8[u], c, m, bad);
            a8[u] = m;
            u8[u] = c;
        }
        store_chunk<DIR, N>(minv + at, inc, a8);
        store_chunk<DIR, N>(cp + at, inc, u8);
    }
    for (; j < L; ++j) {
        const int64_t at = base + j * inc;
        factor_step(lo[at], minv[at], cp[at], c, m, bad);
        minv[at] = m;
        cp[at] = c;
    }
    if (bad) atomicOr(flags, 2);
}

// x <- x + omega * T^-1 r on the systems first, first + step, ...: lane t owns system first + t * step.
//   forward   d_0 = r_0 * minv_0,  d_j = (r_j - lo_j * d_(j-1)) * minv_j          (d overwrites r)
//   backward  e_(L-1) = d_(L-1),   e_j = d_j - cp_j * e_(j+1),   x = x + omega * e_j
// Products and sums round separately (the file is built without contraction): the bits of the NumPy twin.  The
// residual was formed before the launch and no other system's rows are read or written, so x is updated in place.
//
// The two passes over the elements [j0, j1) of one system, by the lane that owns it; d carries the chain in and out.
template <int DIR, int N>
__device__ __forceinline__ void lane_forward(int64_t base, int64_t inc, int64_t j0, int64_t j1, const double *lo,
                                             const double *minv, double *r, double &d)
{
    int64_t j = j0;
    for (; j + N <= j1; j += N) {
        const int64_t at = base + j * inc;
        double r8[N], l8[N], m8[N];
        load_chunk<DIR, N>(r + at, inc, r8);
        load_chunk<DIR, N>(lo + at, inc, l8);
        load_chunk<DIR, N>(minv + at, inc, m8);
#pragma unroll
        for (int u = 0; u < N; ++u) {
            d = (r8[u] - l8[u] * d) * m8[u];
            r8[u] = d;
        }
        store_chunk<DIR, N>(r + at, inc, r8);
    }
    if constexpr (N > kFactorChunk) {                           // what is left of a long block: short blocks, then single elements
        lane_forward<DIR, kFactorChunk>(base, inc, j, j1, lo, minv, r, d);
        return;
    }
    for (; j < j1; ++j) {
        const int64_t at = base + j * inc;
        d = (r[at] - lo[at] * d) * minv[at];
        r[at] = d;
    }
}

template <int DIR, int N>
__device__ __forceinline__ void lane_backward(int64_t base, int64_t inc, int64_t j0, int64_t j1, const double *cp,
                                              const double *r, double omega, double *x, double &d)
{
    int64_t j = j1;                                             // elements j - 1, j - 2, ... down to j0
    for (; j - N >= j0; j -= N) {
        const int64_t at = base + (j - N) * inc;
        double d8[N], c8[N], x8[N];
        load_chunk<DIR, N>(r + at, inc, d8);
        load_chunk<DIR, N>(cp + at, inc, c8);
        load_chunk<DIR, N>(x + at, inc, x8);
#pragma unroll
        for (int u = N - 1; u >= 0; --u) {
            d = d8[u] - c8[u] * d;
            x8[u] = x8[u] + omega * d;
        }
        store_chunk<DIR, N>(x + at, inc, x8);
    }
    if constexpr (N > kFactorChunk) {
        lane_backward<DIR, kFactorChunk>(base, inc, j0, j, cp, r, omega, x, d);
        return;
    }
    for (; j > j0; --j) {
        const int64_t at = base + (j - 1) * inc;
        d = r[at] - cp[at] * d;
        x[at] = x[at] + omega * d;
    }
}

template <int DIR, int N>
__global__ void __launch_bounds__(kLineBlock) line_solve_kernel(int64_t nsys, int64_t L, int64_t W, int64_t first,
                                                                int64_t step, const double *lo, const double *minv,
                                                                const double *cp, double *r, double omega, double *x)
{
    const int64_t k = first + ((int64_t)blockIdx.x * kLineBlock + threadIdx.x) * step;
    if (k >= nsys) return;
    const int64_t base = DIR == DIR_X ? k * W : k, inc = DIR == DIR_X ? 1 : W;
    double d = r[base] * minv[base];                            // d_0 = r_0 * minv_0
    r[base] = d;
    lane_forward<DIR, N>(base, inc, 1, L, lo, minv, r, d);
    const int64_t last = base + (L - 1) * inc;
    x[last] = x[last] + omega * d;                              // e_(L-1) = d_(L-1)
    lane_backward<DIR, N>(base, inc, 0, L - 1, cp, r, omega, x, d);
}

// ---- banded systems: half-bandwidth P = 2 (25-point levels) or 3 (49-point levels) ------------------------------------
// The factors are 2 P + 1 planes of n doubles, each indexed by row like lo / minv / cp above: plane t - 1 holds the
// multiplier l_(j,t) of row j for row j - t (t = 1 .. P), plane P holds minv_j = 1 / u_(j,0), plane P + q the upper entry
// u_(j,q) (q = 1 .. P).  Before the factorisation the same planes hold the band itself: a_(j,j-t), a_(j,j), a_(j,j+q).
// Rows before the first and behind the last of a system count as zero rows (all entries, minv, d and e zero): every row
// runs the same P steps, and the lane starts its chains from zeros.

// The band of every row from the sorted CSR.  Direction x: the entries at column - row = m, |m| <= P, that stay inside the
// row's line; one that leaves it belongs to no system, and a non-zero one sets bit 0 of *flags.  Direction y: the entries
// at column - row = c * W, |c| <= P.  A missing entry is 0; every other entry of the row is not looked at.
template <int DIR, int P>
__global__ void __launch_bounds__(kBlock) band_extract_kernel(int64_t n, int64_t W, const int *rowptr, const int *colidx,
                                                              const double *vals, double *fac, int *flags)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t s = DIR == DIR_X ? 1 : W;
    bool coupled = false;
    for (int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x; row < n; row += stride) {
        double w[2 * P + 1];
#pragma unroll
        for (int m = 0; m <= 2 * P; ++m) w[m] = 0.0;
        for (int e = rowptr[row]; e < rowptr[row + 1]; ++e) {
            const int64_t off = (int64_t)colidx[e] - row;
            const double v = vals[e];
#pragma unroll
            for (int m = -P; m <= P; ++m)
                if (off == m * s) w[m + P] = v;
        }
        if (DIR == DIR_X) {
            const int64_t col = row % W;
#pragma unroll
            for (int m = -P; m <= P; ++m)
                if (m != 0 && (col + m < 0 || col + m >= W)) {
                    coupled |= (w[m + P] != 0.0);
                    w[m + P] = 0.0;
                }
        }
#pragma unroll
        for (int t = 1; t <= P; ++t) fac[(int64_t)(t - 1) * n + row] = w[P - t];
#pragma unroll
        for (int q = 0; q <= P; ++q) fac[(int64_t)(P + q) * n + row] = w[P + q];
    }
    if (coupled) atomicOr(flags, 1);
}

// What a lane carries of the P rows before the one it works on: up[t - 1][q - 1] = u_(j-t,q), mv[t - 1] = minv_(j-t).
template <int P>
struct BandCarry {
    double up[P][P];
    double mv[P];
};

// One row of the factorisation.  w[0 .. 2P] = the band of row j (w[P] the diagonal).  For t = P .. 1, the rows j - P .. j - 1
// in that order:  l_t = w[P - t] * minv_(j-t),  then  w[P - t + q] = w[P - t + q] - l_t * u_(j-t,q)  for q = 1 .. P.  What is
// left is l (l[t - 1] = l_t), the upper row w[P .. 2P] and minv = 1 / w[P]; the carry moves on by one row.
template <int P>
__device__ __forceinline__ void band_factor_step(double (&w)[2 * P + 1], double (&l)[P], double &minv, BandCarry<P> &c,
                                                 bool &bad)
{
#pragma unroll
    for (int t = P; t >= 1; --t) {
        const double lt = w[P - t] * c.mv[t - 1];
#pragma unroll
        for (int q = 1; q <= P; ++q) w[P - t + q] = w[P - t + q] - lt * c.up[t - 1][q - 1];
        l[t - 1] = lt;
    }
    bad |= !(w[P] != 0.0 && fabs(w[P]) <= 1.79769313486231570815e+308);      // zero, infinite or NaN
    minv = 1.0 / w[P];
#pragma unroll
    for (int t = P; t >= 2; --t) {
        c.mv[t - 1] = c.mv[t - 2];
#pragma unroll
        for (int q = 0; q < P; ++q) c.up[t - 1][q] = c.up[t - 2][q];
    }
    c.mv[0] = minv;
#pragma unroll
    for (int q = 0; q < P; ++q) c.up[0][q] = w[P + 1 + q];
}

// The factorisation along every system, in place in the 2 P + 1 planes.  Lane <-> system.
template <int DIR, int P>
__global__ void __launch_bounds__(kLineBlock) band_recur_kernel(int64_t nsys, int64_t L, int64_t W, int64_t n, double *fac,
                                                                int *flags)
{
    constexpr int N = kBandFactorChunk, NP = 2 * P + 1;
    const int64_t k = (int64_t)blockIdx.x * kLineBlock + threadIdx.x;
    if (k >= nsys) return;
    const int64_t base = DIR == DIR_X ? k * W : k, inc = DIR == DIR_X ? 1 : W;
    bool bad = false;
    BandCarry<P> c;
#pragma unroll
    for (int t = 0; t < P; ++t) {
        c.mv[t] = 0.0;
#pragma unroll
        for (int q = 0; q < P; ++q) c.up[t][q] = 0.0;
    }
    int64_t j = 0;
    for (; j + N <= L; j += N) {
        const int64_t at = base + j * inc;
        double b[NP][N];
#pragma unroll
        for (int s = 0; s < NP; ++s) load_chunk<DIR, N>(fac + (int64_t)s * n + at, inc, b[s]);
#pragma unroll
        for (int u = 0; u < N; ++u) {
            double w[NP], l[P], m;
#pragma unroll
            for (int t = 1; t <= P; ++t) w[P - t] = b[t - 1][u];
#pragma unroll
            for (int q = 0; q <= P; ++q) w[P + q] = b[P + q][u];
            band_factor_step<P>(w, l, m, c, bad);
#pragma unroll
            for (int t = 1; t <= P; ++t) b[t - 1][u] = l[t - 1];
            b[P][u] = m;
#pragma unroll
            for (int q = 1; q <= P; ++q) b[P + q][u] = w[P + q];
        }
#pragma unroll
        for (int s = 0; s < NP; ++s) store_chunk<DIR, N>(fac + (int64_t)s * n + at, inc, b[s]);
    }
    for (; j < L; ++j) {
        const int64_t at = base + j * inc;
        double w[NP], l[P], m;
#pragma unroll
        for (int t = 1; t <= P; ++t) w[P - t] = fac[(int64_t)(t - 1) * n + at];
#pragma unroll
        for (int q = 0; q <= P; ++q) w[P + q] = fac[(int64_t)(P + q) * n + at];
        band_factor_step<P>(w, l, m, c, bad);
#pragma unroll
        for (int t = 1; t <= P; ++t) fac[(int64_t)(t - 1) * n + at] = l[t - 1];
        fac[(int64_t)P * n + at] = m;
#pragma unroll
        for (int q = 1; q <= P; ++q) fac[(int64_t)(P + q) * n + at] = w[P + q];
    }
    if (bad) atomicOr(flags, 2);
}

// x <- x + omega * B^-1 r on the systems first, first + step, ..., B = L U the banded part:
//   forward   s = r_j;  s = s - l_(j,t) * d_(j-t) for t = P .. 1;  d_j = s                       (d overwrites r)
//   backward  s = d_j;  s = s - u_(j,q) * e_(j+q) for q = P .. 1;  e_j = s * minv_j;  x_j = x_j + omega * e_j
// The farthest row is subtracted first, so the newest link of the chain enters last.  d[t - 1] carries d_(j-t) in and
// out (e[q - 1] = e_(j+q) in the backward pass); the lane starts both from zeros.
template <int DIR, int P, int N>
__device__ __forceinline__ void band_forward(int64_t base, int64_t inc, int64_t n, int64_t j0, int64_t j1, const double *fac,
                                             double *r, double (&d)[P])
{
    int64_t j = j0;
    for (; j + N <= j1; j += N) {
        const int64_t at = base + j * inc;
        double rN[N], lN[P][N];
        load_chunk<DIR, N>(r + at, inc, rN);
#pragma unroll
        for (int t = 0; t < P; ++t) load_chunk<DIR, N>(fac + (int64_t)t * n + at, inc, lN[t]);
        __builtin_amdgcn_sched_barrier(0);                      // every load of the block is issued before the chain starts
#pragma unroll
        for (int u = 0; u < N; ++u) {
            double s = rN[u];
#pragma unroll
            for (int t = P; t >= 1; --t) s = s - lN[t - 1][u] * d[t - 1];
#pragma unroll
            for (int t = P; t >= 2; --t) d[t - 1] = d[t - 2];
            d[0] = s;
            rN[u] = s;
        }
        store_chunk<DIR, N>(r + at, inc, rN);
    }
    if constexpr (N > kBandShort) {                             // what is left of a long block: short blocks, then single elements
        band_forward<DIR, P, kBandShort>(base, inc, n, j, j1, fac, r, d);
        return;
    }
    for (; j < j1; ++j) {
        const int64_t at = base + j * inc;
        double s = r[at];
#pragma unroll
        for (int t = P; t >= 1; --t) s = s - fac[(int64_t)(t - 1) * n + at] * d[t - 1];
#pragma unroll
        for (int t = P; t >= 2; --t) d[t - 1] = d[t - 2];
        d[0] = s;
        r[at] = s;
    }
}

template <int DIR, int P, int N>
__device__ __forceinline__ void band_backward(int64_t base, int64_t inc, int64_t n, int64_t j0, int64_t j1, const double *fac,
                                              const double *r, double omega, double *x, double (&e)[P])
{
    int64_t j = j1;                                             // elements j - 1, j - 2, ... down to j0
    for (; j - N >= j0; j -= N) {
        const int64_t at = base + (j - N) * inc;
        double dN[N], mN[N], uN[P][N], xN[N];
        load_chunk<DIR, N>(r + at, inc, dN);
        load_chunk<DIR, N>(fac + (int64_t)P * n + at, inc, mN);
#pragma unroll
        for (int q = 0; q < P; ++q) load_chunk<DIR, N>(fac + (int64_t)(P + 1 + q) * n + at, inc, uN[q]);
        load_chunk<DIR, N>(x + at, inc, xN);
        __builtin_amdgcn_sched_barrier(0);                      // (left to itself the scheduler of P = 2, direction y sinks the loads
                                                                //  into the chain, each behind a full wait: three times the time)
#pragma unroll
        for (int u = N - 1; u >= 0; --u) {
            double s = dN[u];
#pragma unroll
            for (int q = P; q >= 1; --q) s = s - uN[q - 1][u] * e[q - 1];
            s = s * mN[u];
#pragma unroll
            for (int q = P; q >= 2; --q) e[q - 1] = e[q - 2];
            e[0] = s;
            xN[u] = xN[u] + omega * s;
        }
        store_chunk<DIR, N>(x + at, inc, xN);
    }
    if constexpr (N > kBandShort) {
        band_backward<DIR, P, kBandShort>(base, inc, n, j0, j, fac, r, omega, x, e);
        return;
    }
    for (; j > j0; --j) {
        const int64_t at = base + (j - 1) * inc;
        double s = r[at];
#pragma unroll
        for (int q = P; q >= 1; --q) s = s - fac[(int64_t)(P + q) * n + at] * e[q - 1];
        s = s * fac[(int64_t)P * n + at];
#pragma unroll
        for (int q = P; q >= 2; --q) e[q - 1] = e[q - 2];
        e[0] = s;
        x[at] = x[at] + omega * s;
    }
}

template <int DIR, int P, int N>
__global__ void __launch_bounds__(kLineBlock) band_solve_kernel(int64_t nsys, int64_t L, int64_t W, int64_t n, int64_t first,
                                                                int64_t step, const double *fac, double *r, double omega,
                                                                double *x)
{
    const int64_t k = first + ((int64_t)blockIdx.x * kLineBlock + threadIdx.x) * step;
    if (k >= nsys) return;
    const int64_t base = DIR == DIR_X ? k * W : k, inc = DIR == DIR_X ? 1 : W;
    double c[P];
#pragma unroll
    for (int t = 0; t < P; ++t) c[t] = 0.0;
    band_forward<DIR, P, N>(base, inc, n, 0, L, fac, r, c);
#pragma unroll
    for (int t = 0; t < P; ++t) c[t] = 0.0;
    band_backward<DIR, P, N>(base, inc, n, 0, L, fac, r, omega, x, c);
}

inline unsigned grid_for(int64_t count, int per_block, int64_t cap)
{
    int64_t g = (count + per_block - 1) / per_block;
    if (cap > 0 && g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace

int lmg_line_factor(int64_t n, int32_t line_stride, int dir, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                    double *lo, double *minv, double *cp, int32_t *flags, void *stream)
{
    if (n < 0 || n >= INT32_MAX || line_stride < 1 || (dir != DIR_X && dir != DIR_Y) || n % line_stride != 0 || !flags)
        return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!rowptr || !colidx || !vals || !lo || !minv || !cp || lo == minv || lo == cp || minv == cp) return LMG_ERR_ARG;
    const int64_t W = line_stride, H = n / W;
    const int64_t nsys = dir == DIR_X ? H : W, L = dir == DIR_X ? W : H;
    hipStream_t st = lmg_stream(stream);
    const unsigned ge = grid_for(n, kBlock, kMaxGrid), gr = grid_for(nsys, kLineBlock, 0);
    if (dir == DIR_X) {
        hipLaunchKernelGGL(line_extract_kernel<DIR_X>, dim3(ge), dim3(kBlock), 0, st, n, W, rowptr, colidx, vals, lo, minv, cp, flags);
        hipLaunchKernelGGL(line_recur_kernel<DIR_X>, dim3(gr), dim3(kLineBlock), 0, st, nsys, L, W, lo, minv, cp, flags);
    } else {
        hipLaunchKernelGGL(line_extract_kernel<DIR_Y>, dim3(ge), dim3(kBlock), 0, st, n, W, rowptr, colidx, vals, lo, minv, cp, flags);
        hipLaunchKernelGGL(line_recur_kernel<DIR_Y>, dim3(gr), dim3(kLineBlock), 0, st, nsys, L, W, lo, minv, cp, flags);
    }
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_line_solve(int64_t n, int32_t line_stride, int dir, int64_t first, int64_t step, const double *lo, const double *minv,
                   const double *cp, double *r, double omega, double *x, void *stream)
{
    if (n < 0 || n >= INT32_MAX || line_stride < 1 || (dir != DIR_X && dir != DIR_Y) || n % line_stride != 0 || first < 0 ||
        step < 1)
        return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!lo || !minv || !cp || !r || !x || r == x || r == lo || r == minv || r == cp || x == lo || x == minv || x == cp)
        return LMG_ERR_ARG;
    const int64_t W = line_stride, H = n / W;
    const int64_t nsys = dir == DIR_X ? H : W, L = dir == DIR_X ? W : H;
    if (first >= nsys) return LMG_OK;
    if (step > nsys) step = nsys;          // (one system either way; keeps first + t * step far from overflow)
    const int64_t count = (nsys - first + step - 1) / step;
    const unsigned grid = grid_for(count, kLineBlock, 0);
    if (dir == DIR_X)
        hipLaunchKernelGGL((line_solve_kernel<DIR_X, kSolveChunkX>), dim3(grid), dim3(kLineBlock), 0, lmg_stream(stream), nsys, L,
                           W, first, step, lo, minv, cp, r, omega, x);
    else
        hipLaunchKernelGGL((line_solve_kernel<DIR_Y, kSolveChunkY>), dim3(grid), dim3(kLineBlock), 0, lmg_stream(stream), nsys, L,
                           W, first, step, lo, minv, cp, r, omega, x);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

namespace {

template <int P>
void launch_band_factor(int dir, unsigned ge, unsigned gr, hipStream_t st, int64_t n, int64_t W, int64_t nsys, int64_t L,
                        const int *rowptr, const int *colidx, const double *vals, double *fac, int *flags)
{
    if (dir == DIR_X) {
        hipLaunchKernelGGL((band_extract_kernel<DIR_X, P>), dim3(ge), dim3(kBlock), 0, st, n, W, rowptr, colidx, vals, fac, flags);
        hipLaunchKernelGGL((band_recur_kernel<DIR_X, P>), dim3(gr), dim3(kLineBlock), 0, st, nsys, L, W, n, fac, flags);
    } else {
        hipLaunchKernelGGL((band_extract_kernel<DIR_Y, P>), dim3(ge), dim3(kBlock), 0, st, n, W, rowptr, colidx, vals, fac, flags);
        hipLaunchKernelGGL((band_recur_kernel<DIR_Y, P>), dim3(gr), dim3(kLineBlock), 0, st, nsys, L, W, n, fac, flags);
    }
}

template <int P>
void launch_band_solve(int dir, unsigned grid, hipStream_t st, int64_t n, int64_t W, int64_t nsys, int64_t L, int64_t first,
                       int64_t step, const double *fac, double *r, double omega, double *x)
{
    if (dir == DIR_X)
        hipLaunchKernelGGL((band_solve_kernel<DIR_X, P, kSolveChunkX>), dim3(grid), dim3(kLineBlock), 0, st, nsys, L, W, n, first,
                           step, fac, r, omega, x);
    else
        hipLaunchKernelGGL((band_solve_kernel<DIR_Y, P, kSolveChunkY>), dim3(grid), dim3(kLineBlock), 0, st, nsys, L, W, n, first,
                           step, fac, r, omega, x);
}

// whether the n doubles at v overlap the planes of fac
inline bool in_planes(const double *v, const double *fac, int64_t n, int band)
{
    return v + n > fac && v < fac + (int64_t)(2 * band + 1) * n;
}

}  // namespace

int lmg_line_factor_banded(int64_t n, int32_t line_stride, int dir, int band, const int32_t *rowptr, const int32_t *colidx,
                           const double *vals, double *fac, int32_t *flags, void *stream)
{
    if (n < 0 || n >= INT32_MAX || line_stride < 1 || (dir != DIR_X && dir != DIR_Y) || band < 2 || band > 3 ||
        n % line_stride != 0 || !flags)
        return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!rowptr || !colidx || !vals || !fac || fac == vals) return LMG_ERR_ARG;
    const int64_t W = line_stride, H = n / W;
    const int64_t nsys = dir == DIR_X ? H : W, L = dir == DIR_X ? W : H;
    hipStream_t st = lmg_stream(stream);
    const unsigned ge = grid_for(n, kBlock, kMaxGrid), gr = grid_for(nsys, kLineBlock, 0);
    if (band == 2)
        launch_band_factor<2>(dir, ge, gr, st, n, W, nsys, L, rowptr, colidx, vals, fac, flags);
    else
        launch_band_factor<3>(dir, ge, gr, st, n, W, nsys, L, rowptr, colidx, vals, fac, flags);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_line_solve_banded(int64_t n, int32_t line_stride, int dir, int band, int64_t first, int64_t step, const double *fac,
                          double *r, double omega, double *x, void *stream)
{
    if (n < 0 || n >= INT32_MAX || line_stride < 1 || (dir != DIR_X && dir != DIR_Y) || band < 2 || band > 3 ||
        n % line_stride != 0 || first < 0 || step < 1)
        return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!fac || !r || !x || r == x || in_planes(r, fac, n, band) || in_planes(x, fac, n, band)) return LMG_ERR_ARG;
    const int64_t W = line_stride, H = n / W;
    const int64_t nsys = dir == DIR_X ? H : W, L = dir == DIR_X ? W : H;
    if (first >= nsys) return LMG_OK;
    if (step > nsys) step = nsys;          // (one system either way; keeps first + t * step far from overflow)
    const int64_t count = (nsys - first + step - 1) / step;
    const unsigned grid = grid_for(count, kLineBlock, 0);
    if (band == 2)
        launch_band_solve<2>(dir, grid, lmg_stream(stream), n, W, nsys, L, first, step, fac, r, omega, x);
    else
        launch_band_solve<3>(dir, grid, lmg_stream(stream), n, W, nsys, L, first, step, fac, r, omega, x);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}
