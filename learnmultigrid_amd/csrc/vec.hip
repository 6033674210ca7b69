// Vector kernels (axpby, products, dot), gather / scatter (halo pack / unpack, coarse permutation), Gershgorin bound,
// pattern parity counts, scan, the list of the tune tables, hipGraph helpers, and the status / version entry points of the
// C ABI.  The dense kernels of the coarse solve are dense.hip.
#include "lmg_common.hpp"

namespace {

// y = alpha*x + beta*y, two elements (16 bytes) per lane per step.
__global__ void __launch_bounds__(kLmgBlock) axpby_kernel(int64_t n, double alpha, const double *x,
                                                          double beta, double *y)
{
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kLmgBlock;
    const double2 *x2 = reinterpret_cast<const double2 *>(x);
    double2 *y2 = reinterpret_cast<double2 *>(y);
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n2; i += stride) {
        const double2 xv = x2[i];
        double2 yv;
        if (beta == 0.0) {
            yv.x = alpha * xv.x;
            yv.y = alpha * xv.y;
        } else {
            yv = y2[i];
            yv.x = alpha * xv.x + beta * yv.x;
            yv.y = alpha * xv.y + beta * yv.y;
        }
        y2[i] = yv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        y[i] = (beta == 0.0) ? alpha * x[i] : alpha * x[i] + beta * y[i];
    }
}

// out = alpha * (x * y) elementwise: the first Jacobi sweep from a zero initial guess,
// x_1 = omega * (D^-1 b), bit-identical to the general sweep with x_0 = 0.
__global__ void __launch_bounds__(kLmgBlock) vmul_kernel(int64_t n, double alpha, const double *x,
                                                         const double *y, double *out)
{
    const int64_t stride = (int64_t)gridDim.x * kLmgBlock;
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n; i += stride)
        out[i] = alpha * (x[i] * y[i]);
}

// One step of the Chebyshev polynomial smoother for the formats without a fused pass, after their residual launch:
//     d = a * d + c * (dinv * r)   (FIRST: d = c * (dinv * r), d is not read),   x = x + d
// two elements (16 bytes) per lane per step; products and sums round separately, the bits of the fused passes.
template <bool FIRST>
__global__ void __launch_bounds__(kLmgBlock) cheby_update_kernel(int64_t n, double a, double c, const double *dinv,
                                                                 const double *r, double *d, double *x)
{
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kLmgBlock;
    const double2 *dinv2 = reinterpret_cast<const double2 *>(dinv), *r2 = reinterpret_cast<const double2 *>(r);
    double2 *d2 = reinterpret_cast<double2 *>(d), *x2 = reinterpret_cast<double2 *>(x);
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n2; i += stride) {
        const double2 iv = dinv2[i], rv = r2[i];
        double2 xv = x2[i], dv;
        if (FIRST) {
            dv.x = c * (iv.x * rv.x);
            dv.y = c * (iv.y * rv.y);
        } else {
            dv = d2[i];
            dv.x = a * dv.x + c * (iv.x * rv.x);
            dv.y = a * dv.y + c * (iv.y * rv.y);
        }
        xv.x = xv.x + dv.x;
        xv.y = xv.y + dv.y;
        d2[i] = dv;
        x2[i] = xv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = n - 1;
        const double z = c * (dinv[i] * r[i]);
        const double dv = FIRST ? z : a * d[i] + z;
        d[i] = dv;
        x[i] = x[i] + dv;
    }
}

// Gershgorin bound of D^-1 A: max over the rows with a non-zero diagonal of (sum_j |a_ij|) / |a_ii|, the row sums in
// storage order (duplicate diagonal entries are summed like lmg_csr_inverse_diagonal does).  The ratios are >= 0, so
// their order as doubles is the order of their bit patterns as unsigned integers: one integer maximum per wave into
// *out (zeroed before the launch) -- a maximum does not depend on the order it is taken in.
__global__ void __launch_bounds__(kLmgBlock) csr_gershgorin_kernel(int64_t n, const int *rowptr, const int *colidx,
                                                                   const double *vals, unsigned long long *out)
{
    const int64_t stride = (int64_t)gridDim.x * kLmgBlock;
    double m = 0.0;
    for (int64_t row = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; row < n; row += stride) {
        double sum = 0.0, dg = 0.0;
        for (int e = rowptr[row]; e < rowptr[row + 1]; ++e) {
            const double v = vals[e];
            sum += fabs(v);
            if (colidx[e] == row) dg += v;
        }
        if (dg != 0.0) {
            const double q = sum / fabs(dg);
            m = q > m ? q : m;                       // (a NaN ratio never wins)
        }
    }
#pragma unroll
    for (int off = LMG_WAVE / 2; off > 0; off >>= 1) {
        const double o = __shfl_down(m, off, LMG_WAVE);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & (LMG_WAVE - 1)) == 0 && m > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(m));
}

// fixed geometry (1024 partials) so the result does not depend on tuning knobs
__global__ void __launch_bounds__(kLmgBlock) dot_kernel(int64_t n, const double *x, const double *y,
                                                        double *partial)
{
    __shared__ double s_red[kLmgBlock / LMG_WAVE];
    double v = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kLmgBlock;
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n; i += stride) v += x[i] * y[i];
    const double tot = lmg_block_sum<kLmgBlock>(v, s_red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(1024) dot_final_kernel(const double *partial, int count, double *out)
{
    __shared__ double s_red[1024 / LMG_WAVE];
    double v = (int)threadIdx.x < count ? partial[threadIdx.x] : 0.0;
    const double tot = lmg_block_sum<1024>(v, s_red);
    if (threadIdx.x == 0) out[0] = tot;
}

__global__ void __launch_bounds__(kLmgBlock) gather_kernel(int64_t n, const int *idx, const double *x,
                                                           double *buf)
{
    const int64_t stride = (int64_t)gridDim.x * kLmgBlock;
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n; i += stride) buf[i] = x[idx[i]];
}

__global__ void __launch_bounds__(kLmgBlock) scatter_kernel(int64_t n, const int *idx, const double *buf,
                                                            double *x)
{
    const int64_t stride = (int64_t)gridDim.x * kLmgBlock;
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n; i += stride) x[idx[i]] = buf[i];
}

// How often every pattern id occurs on (even / odd line) x (even / odd column) of a grid with line stride W:
// counts[((y & 1) * 2 + (x & 1)) * 256 + id] (zeroed by the caller).  Setup helper of ops.ProlongTwin (a library
// histogram costs 0.4 s of code-object loading in a fresh process).
__global__ void __launch_bounds__(kLmgBlock) pattern_parity_counts_kernel(int64_t n, int W, const unsigned char *pid, int *counts)
{
    __shared__ int s_cnt[4 * 256];
    for (int i = threadIdx.x; i < 4 * 256; i += kLmgBlock) s_cnt[i] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLmgBlock) {
        const unsigned y = (unsigned)(i / W), x = (unsigned)(i - (int64_t)y * W);
        atomicAdd(&s_cnt[(((y & 1u) << 1) | (x & 1u)) * 256 + pid[i]], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * 256; i += kLmgBlock)
        if (s_cnt[i]) atomicAdd(&counts[i], s_cnt[i]);
}

// ---- census of the rows that do not hold the expected pattern (table layout: lmg_common.hpp) --------------------------
// First launch: one wave per table row.  Wave 0 clears the border row; wave y + 1 counts line y -- lane l the cell
// 64 k + l in round k -- and writes the running sum along the line.  expect: the id wanted at (line parity, column parity),
// packed one byte each in the order 00, 01, 10, 11; bit 8 + k of `none` set: nothing is wanted there (every row counts).
__global__ void __launch_bounds__(kLmgBlock) pattern_census_lines_kernel(int64_t n, int W, int lines, const unsigned char *pid,
                                                                         unsigned expect, unsigned none, int *table)
{
    const int lane = threadIdx.x & (LMG_WAVE - 1);
    const int row = (int)blockIdx.x * (kLmgBlock / LMG_WAVE) + (int)(threadIdx.x / LMG_WAVE);
    if (row > lines) return;
    const int cells = lmg_census_cells(W);
    int *out = table + (int64_t)row * (cells + 1);
    if (row == 0) {
        for (int c = lane; c <= cells; c += LMG_WAVE) out[c] = 0;
        return;
    }
    const int y = row - 1;
    if (lane == 0) out[0] = 0;
    int carry = 0;
    for (int cb = 0; cb < cells; cb += LMG_WAVE) {
        const int c = cb + lane;
        int bad = 0;
        if (c < cells) {
            for (int k = 0; k < kLmgCensusCell; ++k) {
                const int x = c * kLmgCensusCell + k;
                const int64_t i = (int64_t)y * W + x;
                const int par = ((y & 1) << 1) | (x & 1);
                const bool ok = x < W && i < n && !((none >> par) & 1u) && pid[i] == ((expect >> (8 * par)) & 0xffu);
                bad += ok ? 0 : 1;
            }
        }
        // inclusive sum over the lanes, then the cells of the rounds before
        for (int d = 1; d < LMG_WAVE; d <<= 1) {
            const int up = __shfl_up(bad, d, LMG_WAVE);
            if (lane >= d) bad += up;
        }
        if (c < cells) out[c + 1] = carry + bad;
        carry += __shfl(bad, LMG_WAVE - 1, LMG_WAVE);
    }
}

// Second launch: one thread per table column sums down the lines, eight loads in flight.
__global__ void __launch_bounds__(kLmgBlock) pattern_census_columns_kernel(int lines, int cells, int *table)
{
    const int c = (int)blockIdx.x * kLmgBlock + (int)threadIdx.x + 1;
    if (c > cells) return;
    const int64_t cs = cells + 1;
    int sum = 0;
    for (int y0 = 1; y0 <= lines; y0 += 8) {
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = y0 + k <= lines ? table[(int64_t)(y0 + k) * cs + c] : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            sum += v[k];
            if (y0 + k <= lines) table[(int64_t)(y0 + k) * cs + c] = sum;
        }
    }
}

// ---- exclusive scan (int32): per-block scan + block sums + add-back -------------------
constexpr int kScanBlock = 1024;
constexpr int kScanItems = 4;
constexpr int kScanTile = kScanBlock * kScanItems;

__device__ __forceinline__ int wave_incl_scan(int v, int lane)
{
#pragma unroll
    for (int off = 1; off < LMG_WAVE; off <<= 1) {
        const int u = __shfl_up(v, off, LMG_WAVE);
        if (lane >= off) v += u;
    }
    return v;
}

// scans one tile; out[i+1] receives the inclusive value (caller pre-writes out[0] = 0)
__global__ void __launch_bounds__(kScanBlock) scan_tile_kernel(int64_t n, const int *in, int *out,
                                                               int *block_sums)
{
    __shared__ int s_wave[kScanBlock / LMG_WAVE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)t * kScanItems;
    int v[kScanItems];
    int sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        v[k] = (base + k < n) ? in[base + k] : 0;
        sum += v[k];
    }
    const int incl = wave_incl_scan(sum, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        const int w = (lane < kScanBlock / LMG_WAVE) ? s_wave[lane] : 0;
        const int wi = wave_incl_scan(w, lane);
        if (lane < kScanBlock / LMG_WAVE) s_wave[lane] = wi - w;   // exclusive wave offsets
        if (lane == kScanBlock / LMG_WAVE - 1 && block_sums) block_sums[blockIdx.x] = wi;
    }
    __syncthreads();
    int run = s_wave[wave] + incl - sum;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        run += v[k];
        if (base + k < n) out[base + k + 1] = run;
    }
    if (blockIdx.x == 0 && t == 0) out[0] = 0;
}

__global__ void __launch_bounds__(kScanBlock) scan_add_kernel(int64_t n, int *out, const int *block_offs)
{
    const int off = block_offs[blockIdx.x];
    if (off == 0) return;
    const int64_t base = (int64_t)blockIdx.x * kScanTile;
    for (int i = threadIdx.x; i < kScanTile; i += kScanBlock)
        if (base + i < n) out[base + i + 1] += off;
}

int scan_rec(int64_t n, const int *in, int *out, int *scratch, hipStream_t st)
{
    const int64_t blocks = (n + kScanTile - 1) / kScanTile;
    if (blocks <= 1) {
        hipLaunchKernelGGL(scan_tile_kernel, dim3(1), dim3(kScanBlock), 0, st, n, in, out, (int *)nullptr);
        LMG_CHECK_LAUNCH();
        return LMG_OK;
    }
    int *sums = scratch;                 // blocks entries
    int *offs = scratch + blocks;        // blocks + 1 entries (exclusive scan of sums)
    int *rest = offs + blocks + 1;
    hipLaunchKernelGGL(scan_tile_kernel, dim3((unsigned)blocks), dim3(kScanBlock), 0, st, n, in, out, sums);
    LMG_CHECK_LAUNCH();
    int rc = scan_rec(blocks, sums, offs, rest, st);
    if (rc != LMG_OK) return rc;
    hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)blocks), dim3(kScanBlock), 0, st, n, out, offs);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

}  // namespace

extern "C" {

int lmg_version(void) { return LMG_VERSION; }

const char *lmg_status_string(int s)
{
    switch (s) {
    case LMG_OK: return "ok";
    case LMG_ERR_ARG: return "invalid argument";
    case LMG_ERR_ALIGN: return "array base not 16-byte aligned";
    case LMG_ERR_LAUNCH: return "HIP launch/runtime error";
    case LMG_ERR_CAPACITY: return "row exceeds kernel capacity";
    case LMG_ERR_NODEVICE: return "no HIP device";
    default: return "unknown status";
    }
}

int lmg_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return LMG_ERR_NODEVICE;
    return c;
}

// the tune-key table of every file that owns knobs (lmg_common.hpp)
static const LmgTuneKey *const kTuneTables[] = {lmg_tune_sweep, lmg_tune_pcsr,  lmg_tune_rpat, lmg_tune_stencil, lmg_tune_fused,
                                                lmg_tune_tile,  lmg_tune_dia,   lmg_tune_sell, lmg_tune_gsw,     lmg_tune_gs};

static const LmgTuneKey *tune_find(const char *key)
{
    if (!key) return nullptr;
    for (const LmgTuneKey *table : kTuneTables)
        if (const LmgTuneKey *k = lmg_tune_find(table, key)) return k;
    return nullptr;
}

int lmg_tune_set(const char *key, int value)
{
    // The one alias: "rpat_variant" with a value >= 1000 sets "rpat_nt_rows" and leaves the variant alone.  bench.py
    // spells the nontemporal threshold of its LMG_RPAT_NT_ROWS runs this way.
    if (key && strcmp(key, "rpat_variant") == 0 && value >= 1000) key = "rpat_nt_rows";
    const LmgTuneKey *k = tune_find(key);
    if (!k || !lmg_tune_accepts(*k, value)) return LMG_ERR_ARG;
    *k->value = value;
    return LMG_OK;
}

int lmg_tune_get(const char *key)
{
    const LmgTuneKey *k = tune_find(key);
    return k ? *k->value : LMG_ERR_ARG;
}

int lmg_axpby(int64_t n, double alpha, const double *x, double beta, double *y, void *stream)
{
    if (n < 0 || (n > 0 && (!x || !y))) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!lmg_aligned16(x) || !lmg_aligned16(y)) return LMG_ERR_ALIGN;
    hipLaunchKernelGGL(axpby_kernel, dim3(lmg_grid_for(n, kLmgBlock * 2)), dim3(kLmgBlock), 0, lmg_stream(stream),
                       n, alpha, x, beta, y);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_vmul(int64_t n, double alpha, const double *x, const double *y, double *out, void *stream)
{
    if (n < 0 || (n > 0 && (!x || !y || !out))) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    hipLaunchKernelGGL(vmul_kernel, dim3(lmg_grid_for(n, kLmgBlock)), dim3(kLmgBlock), 0, lmg_stream(stream), n, alpha, x, y, out);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_cheby_update(int64_t n, double a, double c, int first, const double *dinv, const double *r, double *d, double *x,
                     void *stream)
{
    if (n < 0 || (n > 0 && (!dinv || !r || !d || !x))) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (d == x || d == r || d == dinv || x == r || x == dinv) return LMG_ERR_ARG;
    if (!lmg_aligned16(dinv) || !lmg_aligned16(r) || !lmg_aligned16(d) || !lmg_aligned16(x)) return LMG_ERR_ALIGN;
    const unsigned grid = lmg_grid_for(n, kLmgBlock * 2);
    if (first)
        hipLaunchKernelGGL(cheby_update_kernel<true>, dim3(grid), dim3(kLmgBlock), 0, lmg_stream(stream), n, a, c, dinv, r, d, x);
    else
        hipLaunchKernelGGL(cheby_update_kernel<false>, dim3(grid), dim3(kLmgBlock), 0, lmg_stream(stream), n, a, c, dinv, r, d, x);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_csr_gershgorin(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, double *lmax, void *stream)
{
    if (n < 0 || n >= INT32_MAX || !lmax || (n > 0 && (!rowptr || !colidx || !vals))) return LMG_ERR_ARG;
    if (hipMemsetAsync(lmax, 0, sizeof(double), lmg_stream(stream)) != hipSuccess) return LMG_ERR_LAUNCH;
    if (n == 0) return LMG_OK;
    hipLaunchKernelGGL(csr_gershgorin_kernel, dim3(lmg_grid_for(n, kLmgBlock)), dim3(kLmgBlock), 0, lmg_stream(stream), n, rowptr, colidx,
                       vals, reinterpret_cast<unsigned long long *>(lmax));
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_copy(int64_t n, const double *src, double *dst, void *stream)
{
    if (n < 0 || (n > 0 && (!src || !dst))) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (hipMemcpyAsync(dst, src, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice,
                       lmg_stream(stream)) != hipSuccess)
        return LMG_ERR_LAUNCH;
    return LMG_OK;
}

int lmg_zero(int64_t n, double *x, void *stream)
{
    if (n < 0 || (n > 0 && !x)) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (hipMemsetAsync(x, 0, (size_t)n * sizeof(double), lmg_stream(stream)) != hipSuccess)
        return LMG_ERR_LAUNCH;
    return LMG_OK;
}

int lmg_dot(int64_t n, const double *x, const double *y, double *partials, double *out, void *stream)
{
    if (n < 0 || !partials || !out || (n > 0 && (!x || !y))) return LMG_ERR_ARG;
    const unsigned grid = 1024;
    hipLaunchKernelGGL(dot_kernel, dim3(grid), dim3(kLmgBlock), 0, lmg_stream(stream), n, x, y, partials);
    LMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(1024), 0, lmg_stream(stream), partials, (int)grid, out);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_gather(int64_t n, const int32_t *idx, const double *x, double *buf, void *stream)
{
    if (n < 0 || (n > 0 && (!idx || !x || !buf))) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    hipLaunchKernelGGL(gather_kernel, dim3(lmg_grid_for(n, kLmgBlock)), dim3(kLmgBlock), 0, lmg_stream(stream), n, idx, x, buf);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_scatter(int64_t n, const int32_t *idx, const double *buf, double *x, void *stream)
{
    if (n < 0 || (n > 0 && (!idx || !x || !buf))) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    hipLaunchKernelGGL(scatter_kernel, dim3(lmg_grid_for(n, kLmgBlock)), dim3(kLmgBlock), 0, lmg_stream(stream), n, idx, buf, x);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_pattern_parity_counts(int64_t n, int32_t line_stride, const uint8_t *pid, int32_t *counts, void *stream)
{
    if (n < 0 || line_stride < 1 || (n > 0 && (!pid || !counts))) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    hipLaunchKernelGGL(pattern_parity_counts_kernel, dim3(lmg_grid_for(n, kLmgBlock * 16)), dim3(kLmgBlock), 0, lmg_stream(stream), n,
                       line_stride, pid, counts);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int64_t lmg_pattern_census_count(int64_t n, int32_t line_stride)
{
    if (n < 1 || line_stride < 1 || (n + line_stride - 1) / line_stride >= INT_MAX) return 0;
    return lmg_census_count((int)((n + line_stride - 1) / line_stride), line_stride);
}

int lmg_pattern_census(int64_t n, int32_t line_stride, const uint8_t *pid, const int32_t *h_expected, int32_t *table, void *stream)
{
    if (n < 0 || n >= (1ll << 31) - 8 || line_stride < 1 || !h_expected || (n > 0 && (!pid || !table))) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    unsigned expect = 0, none = 0;
    for (int k = 0; k < 4; ++k) {
        if (h_expected[k] > 255) return LMG_ERR_ARG;
        if (h_expected[k] < 0) none |= 1u << k;
        else expect |= (unsigned)h_expected[k] << (8 * k);
    }
    const int lines = (int)((n + line_stride - 1) / line_stride), cells = lmg_census_cells(line_stride);
    constexpr int kWaves = kLmgBlock / LMG_WAVE;
    hipLaunchKernelGGL(pattern_census_lines_kernel, dim3((unsigned)((lines + 1 + kWaves - 1) / kWaves)), dim3(kLmgBlock), 0,
                       lmg_stream(stream), n, line_stride, lines, pid, expect, none, table);
    LMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(pattern_census_columns_kernel, dim3((unsigned)((cells + kLmgBlock - 1) / kLmgBlock)), dim3(kLmgBlock), 0,
                       lmg_stream(stream), lines, cells, table);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int64_t lmg_scan_scratch_count(int64_t n)
{
    int64_t total = 0;
    int64_t blocks = (n + kScanTile - 1) / kScanTile;
    while (blocks > 1) {
        total += 2 * blocks + 1;
        blocks = (blocks + kScanTile - 1) / kScanTile;
    }
    return total + 16;
}

int lmg_exclusive_scan_i32(int64_t n, const int32_t *in, int32_t *out, int32_t *scratch, void *stream)
{
    if (n < 0 || !out || (n > 0 && !in)) return LMG_ERR_ARG;
    if (n > kScanTile && !scratch) return LMG_ERR_ARG;
    return scan_rec(n, in, out, scratch, lmg_stream(stream));
}

int lmg_graph_begin(void *stream)
{
    if (hipStreamBeginCapture(lmg_stream(stream), hipStreamCaptureModeThreadLocal) != hipSuccess)
        return LMG_ERR_LAUNCH;
    return LMG_OK;
}

int lmg_graph_end(void *stream, void **exec_out)
{
    if (!exec_out) return LMG_ERR_ARG;
    hipGraph_t g = nullptr;
    if (hipStreamEndCapture(lmg_stream(stream), &g) != hipSuccess || !g) return LMG_ERR_LAUNCH;
    hipGraphExec_t ex = nullptr;
    hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return LMG_ERR_LAUNCH;
    *exec_out = ex;
    return LMG_OK;
}

int lmg_graph_launch(void *exec, void *stream)
{
    if (!exec) return LMG_ERR_ARG;
    if (hipGraphLaunch(reinterpret_cast<hipGraphExec_t>(exec), lmg_stream(stream)) != hipSuccess)
        return LMG_ERR_LAUNCH;
    return LMG_OK;
}

int lmg_graph_destroy(void *exec)
{
    if (!exec) return LMG_OK;
    (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(exec));
    return LMG_OK;
}

}  // extern "C"
