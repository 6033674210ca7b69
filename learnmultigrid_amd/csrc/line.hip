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
#include "lmg_common.hpp"

namespace {

constexpr int kBlock = 256;         // the row-parallel extraction
constexpr int kLineBlock = 64;      // one wave per workgroup: the few dozen waves of a level spread over the CUs
constexpr int kFactorChunk = 8;     // elements per block of loads: the factorisation (setup) and the ends of a solve ...
constexpr int kSolveChunkY = 16;    // ... the solve in direction y: 48 coalesced 8-byte loads in flight per wave ...
constexpr int kSolveChunkX = 32;    // ... and in direction x: 48 loads of 16 bytes per lane
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
