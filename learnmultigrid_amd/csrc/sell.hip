// Sliced-ELL sweeps for gfx950: residual / Jacobi / SpMV on matrices with LONG rows.
//
// The Galerkin operators of L2-type / learned transfer operators have 25-50 entries per row
// with all-distinct values.  pcsr.hip stages a tile's entry stream through LDS and lets lane t
// walk row t; with rows that long a tile of 64 rows already needs ~30 KB of LDS (5 waves per
// CU) and -- worse -- lane t reads LDS at a stride of one ROW (48 entries = 96 dwords: all 64
// lanes land on two banks), so those levels ran at 1.8-3.0 TB/s.  Here the order of the
// entries in memory is changed instead (SELL-64, a lossless re-encoding like PCSR):
//   slice s = rows 64 s .. 64 s + 63, padded to the longest row L_s of the slice;
//   entry j of row r is stored at  slice_base[s] + 64 j + (r mod 64)
// so the wave that owns a slice reads entry j of all its 64 rows with ONE coalesced load per
// stream (columns: uint16 relative to the slice's smallest column when every slice spans
// < 65536 columns, else int32; values: raw fp64, or -- the _f32 entry points -- fp32 widened to fp64
// when loaded), straight into registers: no LDS, no barrier, full occupancy.  Lane t still accumulates row t in storage order with separately rounded
// products => bit-identical to the CSR kernels.  Padding costs (L_s - len) entries per row:
// a few per cent for the near-uniform rows this format is used for.
#include "lmg_common.hpp"
#include <float.h>
#include <limits.h>

namespace {

constexpr int kBlock = 256;
constexpr int kSlicesPerBlock = kBlock / LMG_WAVE;

struct SArgs {
    int n;
    int nslices;
    int nblocks;
    int blocks_per_xcd;
    const long long *slice_base;   // nslices: first padded entry of the slice
    const int *slice_len;          // nslices: padded row length L_s
    const int *slice_cmin;         // nslices: column base (COL16)
    const int *rowlen;             // n
    const void *col;
    const void *val;               // VT of the kernel: double, or float (widened when loaded)
    const double *x;
    const double *b;
    double *out;
    double alpha, beta;
    double *partial;
};

// NT: the entry streams (columns, values) are read once per sweep: nontemporal loads keep them from evicting the
// vector lines the gathers of x live on (L2)
// VT float: the twin represents double(float(A)) value by value -- same products, same order, same diagonal
template <int MODE, bool COL16, int JU, bool NT = false, typename VT = double>
__global__ void __launch_bounds__(kBlock) sell_sweep_kernel(SArgs a)
{
    __shared__ double s_red[kBlock / LMG_WAVE];
    typedef typename std::conditional<COL16, unsigned short, int>::type col_t;
    const col_t *col = static_cast<const col_t *>(a.col);
    const VT *val = static_cast<const VT *>(a.val);
    const int lane = threadIdx.x & (LMG_WAVE - 1), wave = threadIdx.x / LMG_WAVE;
    // XCD-aware: XCD k (blockIdx mod 8) works on the k-th contiguous eighth of the slices
    const int blk = lmg_xcd_tile(a.blocks_per_xcd);
    const int slice = blk * kSlicesPerBlock + wave;
    double local = 0.0;
    if (blk < a.nblocks && slice < a.nslices) {
        const int row = slice * LMG_WAVE + lane;
        const bool valid = row < a.n;
        const int len = valid ? a.rowlen[row] : 0;
        const int slen = a.slice_len[slice];
        const long long base = a.slice_base[slice] + lane;
        const int cb = COL16 ? a.slice_cmin[slice] : 0;
        const double bv = (MODE != MODE_SPMV && valid) ? a.b[row] : 0.0;
        double acc = 0.0, diag = 0.0, xi = 0.0;
        for (int j0 = 0; j0 < slen; j0 += JU) {
            int c[JU];
            double v[JU], xv[JU];
#pragma unroll
            for (int jj = 0; jj < JU; ++jj) {
                const int j = (j0 + jj < slen) ? j0 + jj : slen - 1;      // padded storage: always readable
                const long long e = base + (long long)j * LMG_WAVE;
                c[jj] = cb + (int)(NT ? __builtin_nontemporal_load(col + e) : col[e]);
                v[jj] = (double)(NT ? __builtin_nontemporal_load(val + e) : val[e]);
            }
#pragma unroll
            for (int jj = 0; jj < JU; ++jj) xv[jj] = a.x[(j0 + jj < len) ? c[jj] : 0];
#pragma unroll
            for (int jj = 0; jj < JU; ++jj) {
                const bool act = j0 + jj < len;
                const double s2 = acc + v[jj] * xv[jj];
                acc = act ? s2 : acc;
                if (MODE == MODE_JACOBI) {
                    const bool dg = act && c[jj] == row;
                    diag = dg ? diag + v[jj] : diag;
                    xi = dg ? xv[jj] : xi;
                }
            }
        }
        if (valid) {
            if (MODE == MODE_RESIDUAL) {
                const double r = bv - acc;
                if (a.out) a.out[row] = r;
                local = r * r;
            } else if (MODE == MODE_JACOBI) {
                const double r = bv - acc;
                if (diag != 0.0) a.out[row] = xi + a.alpha * ((1.0 / diag) * r);
                else a.out[row] = a.x[row];
            } else {
                double s = acc;
                if (a.alpha != 1.0) s = a.alpha * s;
                if (a.beta == 0.0) a.out[row] = s;
                else if (a.beta == 1.0) a.out[row] = a.out[row] + s;
                else a.out[row] = a.beta * a.out[row] + s;
            }
        }
    }
    if (MODE == MODE_RESIDUAL && a.partial != nullptr) {
        const double tot = lmg_block_sum<kBlock>(local, s_red);
        if (threadIdx.x == 0 && blk < a.nblocks) a.partial[blk] = tot;
    }
}

// ---- the same sweeps on a block of K vectors ---------------------------------------------------
// X[i * K + j] = row i, column j (K = 2, 4, 8; 16-byte aligned base).  One wave per slice, lane = row as above; an
// entry's column and value are loaded ONCE and serve K accumulators, the K values x[c*K .. c*K + K) come as K/2
// 16-byte loads, and the outputs leave as 16-byte stores: the matrix bytes of a sweep are shared by K columns.
// Column j carries the bits of sell_sweep_kernel run on column j alone: storage order, separately rounded products,
// the same diagonal sum (one per row, whatever the column), diag == 0 -> out = x, the same alpha / beta special cases.
// The Jacobi iterate of the row is read once at the end instead of being carried from the diagonal entry -- the value
// is x[row] either way -- which saves K registers per lane.  norm2[j]: the same lane -> wave -> workgroup sums per column;
// workgroup blk leaves its K sums at partial[blk * K + j].
template <int K>
constexpr int block_ju()
{
    // entries of a row in flight (K doubles of x each): 5 divides the 25-entry rows and leaves one idle slot in ten
    // trips over 49 entries; at K = 8 the gathered values alone are 16 registers per entry -- 4 keeps the kernel at
    // 96 - 102 VGPRs (4 - 5 waves per SIMD, no scratch), see DESIGN.md section 3 (block of right-hand sides)
    return K == 8 ? 4 : 5;
}

template <int MODE, bool COL16, int K, int JU, bool NT>
__global__ void __launch_bounds__(kBlock) sell_sweep_block_kernel(SArgs a)
{
    __shared__ double s_red[K][kBlock / LMG_WAVE];
    constexpr int H = K / 2;                                   // 16-byte pieces of a row of a block
    typedef typename std::conditional<COL16, unsigned short, int>::type col_t;
    const col_t *col = static_cast<const col_t *>(a.col);
    const double *val = static_cast<const double *>(a.val);
    const d2 *x2 = reinterpret_cast<const d2 *>(a.x);
    const int lane = threadIdx.x & (LMG_WAVE - 1), wave = threadIdx.x / LMG_WAVE;
    const int blk = lmg_xcd_tile(a.blocks_per_xcd);
    const int slice = blk * kSlicesPerBlock + wave;
    double local[K];
#pragma unroll
    for (int k = 0; k < K; ++k) local[k] = 0.0;
    if (blk < a.nblocks && slice < a.nslices) {
        const int row = slice * LMG_WAVE + lane;
        const bool valid = row < a.n;
        const int len = valid ? a.rowlen[row] : 0;
        const int slen = a.slice_len[slice];
        const long long base = a.slice_base[slice] + lane;
        const int cb = COL16 ? a.slice_cmin[slice] : 0;
        const long long rbase = (long long)row * H;
        double acc[K], diag = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0.0;
        for (int j0 = 0; j0 < slen; j0 += JU) {
            int c[JU];
            double v[JU];
            d2 xv[JU][H];
#pragma unroll
            for (int jj = 0; jj < JU; ++jj) {
                const int j = (j0 + jj < slen) ? j0 + jj : slen - 1;      // padded storage: always readable
                const long long e = base + (long long)j * LMG_WAVE;
                c[jj] = cb + (int)(NT ? __builtin_nontemporal_load(col + e) : col[e]);
                v[jj] = NT ? __builtin_nontemporal_load(val + e) : val[e];
            }
#pragma unroll
            for (int jj = 0; jj < JU; ++jj) {
                const long long xb = (long long)((j0 + jj < len) ? c[jj] : 0) * H;
#pragma unroll
                for (int h = 0; h < H; ++h) xv[jj][h] = x2[xb + h];
            }
#pragma unroll
            for (int jj = 0; jj < JU; ++jj) {
                const bool act = j0 + jj < len;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double s2 = acc[k] + v[jj] * xv[jj][k / 2][k & 1];
                    acc[k] = act ? s2 : acc[k];
                }
                if (MODE == MODE_JACOBI) diag = (act && c[jj] == row) ? diag + v[jj] : diag;
            }
        }
        if (valid) {
            d2 *o2 = reinterpret_cast<d2 *>(a.out);
            if (MODE == MODE_RESIDUAL) {
                const d2 *b2 = reinterpret_cast<const d2 *>(a.b);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const d2 bv = b2[rbase + h];
                    d2 r;
                    r[0] = bv[0] - acc[2 * h];
                    r[1] = bv[1] - acc[2 * h + 1];
                    if (a.out) o2[rbase + h] = r;
                    local[2 * h] = r[0] * r[0];
                    local[2 * h + 1] = r[1] * r[1];
                }
            } else if (MODE == MODE_JACOBI) {
                const d2 *b2 = reinterpret_cast<const d2 *>(a.b);
                const double rd = 1.0 / diag;
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const d2 bv = b2[rbase + h], xi = x2[rbase + h];
                    d2 o = xi;
                    if (diag != 0.0) {
                        o[0] = xi[0] + a.alpha * (rd * (bv[0] - acc[2 * h]));
                        o[1] = xi[1] + a.alpha * (rd * (bv[1] - acc[2 * h + 1]));
                    }
                    o2[rbase + h] = o;
                }
            } else {
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    d2 s;
                    s[0] = acc[2 * h];
                    s[1] = acc[2 * h + 1];
                    if (a.alpha != 1.0) {
                        s[0] = a.alpha * s[0];
                        s[1] = a.alpha * s[1];
                    }
                    if (a.beta == 1.0) {
                        const d2 y = o2[rbase + h];
                        s[0] = y[0] + s[0];
                        s[1] = y[1] + s[1];
                    } else if (a.beta != 0.0) {
                        const d2 y = o2[rbase + h];
                        s[0] = a.beta * y[0] + s[0];
                        s[1] = a.beta * y[1] + s[1];
                    }
                    o2[rbase + h] = s;
                }
            }
        }
    }
    if (MODE == MODE_RESIDUAL && a.partial != nullptr) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double tot = lmg_block_sum<kBlock>(local[k], s_red[k]);      // (one LDS row per column: no reuse hazard)
            if (threadIdx.x == 0 && blk < a.nblocks) a.partial[(long long)blk * K + k] = tot;
        }
    }
}

// ---- building the format (setup) -------------------------------------------------------------
// one wave per slice: padded length and column range
__global__ void __launch_bounds__(kBlock) sell_slice_info_kernel(int64_t n, int64_t nslices, const int *__restrict__ rowptr,
                                                                 const int *__restrict__ colidx, int *slice_len,
                                                                 int *cmin, int *cmax)
{
    const int lane = threadIdx.x & (LMG_WAVE - 1);
    const int64_t slice = (int64_t)blockIdx.x * kSlicesPerBlock + threadIdx.x / LMG_WAVE;
    if (slice >= nslices) return;
    const int64_t row = slice * LMG_WAVE + lane;
    int len = 0, mn = INT_MAX, mx = 0;
    if (row < n) {
        const int s = rowptr[row], e = rowptr[row + 1];
        len = e - s;
        for (int k = s; k < e; ++k) {
            const int c = colidx[k];
            mn = c < mn ? c : mn;
            mx = c > mx ? c : mx;
        }
    }
#pragma unroll
    for (int off = LMG_WAVE / 2; off > 0; off >>= 1) {
        const int l2 = __shfl_down(len, off, LMG_WAVE), a = __shfl_down(mn, off, LMG_WAVE), b = __shfl_down(mx, off, LMG_WAVE);
        len = l2 > len ? l2 : len;
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (lane == 0) {
        slice_len[slice] = len;
        cmin[slice] = mn == INT_MAX ? 0 : mn;
        cmax[slice] = mx;
    }
}

// lane = row: copies its entries to their padded positions (col_out may be null: values only).  VT float: the values are
// rounded to fp32; *flag |= 1 when a stored value other than 0 is not finite or rounds to +-inf, a subnormal or zero
// (rounding must not change what an entry is: the caller then keeps fp64 values)
template <bool COL16, typename VT>
__global__ void __launch_bounds__(kBlock) sell_fill_kernel(int64_t n, int64_t nslices, const int *__restrict__ rowptr,
                                                           const int *__restrict__ colidx, const double *__restrict__ vals,
                                                           const long long *__restrict__ slice_base,
                                                           const int *__restrict__ cmin, void *col_out, VT *val_out, int *flag)
{
    typedef typename std::conditional<COL16, unsigned short, int>::type col_t;
    col_t *co = static_cast<col_t *>(col_out);
    const int lane = threadIdx.x & (LMG_WAVE - 1);
    const int64_t slice = (int64_t)blockIdx.x * kSlicesPerBlock + threadIdx.x / LMG_WAVE;
    if (slice >= nslices) return;
    const int64_t row = slice * LMG_WAVE + lane;
    if (row >= n) return;
    const int s = rowptr[row], e = rowptr[row + 1];
    const long long base = slice_base[slice] + lane;
    const int cb = COL16 ? cmin[slice] : 0;
    bool bad = false;
    for (int k = s; k < e; ++k) {
        const long long p = base + (long long)(k - s) * LMG_WAVE;
        if (co) co[p] = (col_t)(colidx[k] - cb);
        const double v = vals[k];
        const VT w = (VT)v;
        if (sizeof(VT) == 4) {
            const float m = fabsf((float)w);
            bad = bad || (v != 0.0 && !(m >= FLT_MIN && m <= FLT_MAX));     // (NaN fails both comparisons)
        }
        val_out[p] = w;
    }
    if (bad) atomicOr(flag, 1);
}

// measured (tools/time_sell.py, Jacobi sweep): 2049^2 x 25 entries (1.05 GB) 0.264 -> 0.250 ms, 1025^2 x 49 (0.51 GB)
// 0.122 -> 0.114 ms, but 721^2 x 25 (0.13 GB: the whole matrix stays in the Infinity Cache) 0.025 -> 0.032 ms
int g_sell_ju = 0;                        // entries of a row in flight: 0 = by the longest row (5, 7 or 8); 5, 7, 8, 10 forced
int g_sell_nt = -1;                       // -1: by size, 0: never, 1: always
int64_t g_sell_nt_entries = 30000000;     // padded entries from which the streams no longer fit the 256 MB Infinity Cache

template <int MODE, bool COL16, typename VT>
int launch(SArgs a, int max_len, hipStream_t st)
{
    // measured on MI355X (tools/tune_sweep.py --matrix L1|L2): see DESIGN.md.  The choices below were measured on fp64 values
    // and are kept as they are for fp32 values (sell_nt_entries counts entries, not bytes)
    const dim3 grid((unsigned)(a.blocks_per_xcd * 8)), block(kBlock);
    const bool nt = g_sell_nt == 1 || (g_sell_nt < 0 && (int64_t)a.n * max_len >= g_sell_nt_entries);
    // entries of a row in flight: the factor that leaves the fewest idle slots in the last trip over the longest row (25-entry
    // rows: 5 trips of 5 instead of 4 of 8 -- 2049^2 x 25: 0.2505 -> 0.2290 ms; 49: 7 x 7 -- 1025^2 x 49: 0.1057 -> 0.0982 ms)
    int ju = g_sell_ju;
    if (ju == 0) {
        ju = 8;
        int waste = (8 - max_len % 8) % 8;
        const int cand[2] = {7, 5};
        for (int k = 0; k < 2; ++k) {
            const int w = (cand[k] - max_len % cand[k]) % cand[k];
            if (w < waste) {
                waste = w;
                ju = cand[k];
            }
        }
    }
    if (max_len <= 12) hipLaunchKernelGGL((sell_sweep_kernel<MODE, COL16, 4, false, VT>), grid, block, 0, st, a);
    else if (ju == 5 && nt) hipLaunchKernelGGL((sell_sweep_kernel<MODE, COL16, 5, true, VT>), grid, block, 0, st, a);
    else if (ju == 5) hipLaunchKernelGGL((sell_sweep_kernel<MODE, COL16, 5, false, VT>), grid, block, 0, st, a);
    else if (ju == 7 && nt) hipLaunchKernelGGL((sell_sweep_kernel<MODE, COL16, 7, true, VT>), grid, block, 0, st, a);
    else if (ju == 7) hipLaunchKernelGGL((sell_sweep_kernel<MODE, COL16, 7, false, VT>), grid, block, 0, st, a);
    else if (ju == 10 && nt) hipLaunchKernelGGL((sell_sweep_kernel<MODE, COL16, 10, true, VT>), grid, block, 0, st, a);
    else if (ju == 10) hipLaunchKernelGGL((sell_sweep_kernel<MODE, COL16, 10, false, VT>), grid, block, 0, st, a);
    else if (nt) hipLaunchKernelGGL((sell_sweep_kernel<MODE, COL16, 8, true, VT>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((sell_sweep_kernel<MODE, COL16, 8, false, VT>), grid, block, 0, st, a);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

template <typename VT>
int sell_sweep(int mode, int64_t n, const int64_t *slice_base, const int32_t *slice_len, const int32_t *slice_cmin,
               const int32_t *rowlen, const void *col, int colmode, const VT *val, int32_t max_len, const double *x,
               const double *b, double *out, double alpha, double beta, double *partials, double *norm2, void *stream)
{
    if (n < 0 || n >= INT32_MAX - 64 || (colmode != 0 && colmode != 1) || max_len < 0) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!slice_base || !slice_len || !rowlen || !col || !val || !x) return LMG_ERR_ARG;
    if (colmode == 0 && !slice_cmin) return LMG_ERR_ARG;
    if (lmg_check_sweep_args(mode, x, b, out, partials, norm2) != LMG_OK) return LMG_ERR_ARG;
    SArgs a;
    a.n = (int)n;
    a.nslices = (int)((n + LMG_WAVE - 1) / LMG_WAVE);
    a.nblocks = (a.nslices + kSlicesPerBlock - 1) / kSlicesPerBlock;
    a.blocks_per_xcd = (a.nblocks + 7) / 8;
    a.slice_base = reinterpret_cast<const long long *>(slice_base);
    a.slice_len = slice_len;
    a.slice_cmin = slice_cmin;
    a.rowlen = rowlen;
    a.col = col;
    a.val = val;
    a.x = x;
    a.b = b;
    a.out = out;
    a.alpha = alpha;
    a.beta = beta;
    a.partial = (mode == MODE_RESIDUAL) ? partials : nullptr;
    hipStream_t st = lmg_stream(stream);
    int rc;
    if (colmode == 0) {
        rc = mode == MODE_RESIDUAL ? launch<MODE_RESIDUAL, true, VT>(a, max_len, st)
           : mode == MODE_JACOBI ? launch<MODE_JACOBI, true, VT>(a, max_len, st) : launch<MODE_SPMV, true, VT>(a, max_len, st);
    } else {
        rc = mode == MODE_RESIDUAL ? launch<MODE_RESIDUAL, false, VT>(a, max_len, st)
           : mode == MODE_JACOBI ? launch<MODE_JACOBI, false, VT>(a, max_len, st) : launch<MODE_SPMV, false, VT>(a, max_len, st);
    }
    if (rc != LMG_OK) return rc;
    // blocks beyond nblocks (grid rounded up to a multiple of 8) write nothing: only nblocks partials exist
    if (mode == MODE_RESIDUAL && partials) return lmg_reduce_partials(partials, a.nblocks, norm2, st);
    return LMG_OK;
}

// The block sweep's kernel for (mode, colmode, k, nt): JU is fixed per K (block_ju), there is no tune key of its own.
template <int MODE, bool COL16, int K>
int launch_block(const SArgs &a, bool nt, hipStream_t st)
{
    const dim3 grid((unsigned)(a.blocks_per_xcd * 8)), block(kBlock);
    if (nt) hipLaunchKernelGGL((sell_sweep_block_kernel<MODE, COL16, K, block_ju<K>(), true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((sell_sweep_block_kernel<MODE, COL16, K, block_ju<K>(), false>), grid, block, 0, st, a);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}
template <int MODE, bool COL16>
int launch_block_k(const SArgs &a, int k, bool nt, hipStream_t st)
{
    return k == 2 ? launch_block<MODE, COL16, 2>(a, nt, st)
         : k == 4 ? launch_block<MODE, COL16, 4>(a, nt, st) : launch_block<MODE, COL16, 8>(a, nt, st);
}

inline bool block_width_ok(int k) { return k == 2 || k == 4 || k == 8; }

// flag: the range flag of the fp32 form (null for fp64 values, which the kernel then never touches)
template <typename VT>
int sell_fill(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, const int64_t *slice_base,
              const int32_t *slice_cmin, int colmode, void *col_out, VT *val_out, int32_t *flag, void *stream)
{
    if (n < 0 || (colmode != 0 && colmode != 1)) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!rowptr || !vals || !slice_base || !val_out || (col_out && !colidx) || (colmode == 0 && !slice_cmin))
        return LMG_ERR_ARG;
    if (sizeof(VT) == 4 && !flag) return LMG_ERR_ARG;
    const int64_t nslices = (n + LMG_WAVE - 1) / LMG_WAVE;
    const unsigned grid = (unsigned)((nslices + kSlicesPerBlock - 1) / kSlicesPerBlock);
    const long long *sb = reinterpret_cast<const long long *>(slice_base);
    if (colmode == 0)
        hipLaunchKernelGGL((sell_fill_kernel<true, VT>), dim3(grid), dim3(kBlock), 0, lmg_stream(stream), n, nslices, rowptr,
                           colidx, vals, sb, slice_cmin, col_out, val_out, flag);
    else
        hipLaunchKernelGGL((sell_fill_kernel<false, VT>), dim3(grid), dim3(kBlock), 0, lmg_stream(stream), n, nslices, rowptr,
                           colidx, vals, sb, slice_cmin, col_out, val_out, flag);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

}  // namespace

constexpr LmgTuneKey lmg_tune_sell[] = {
    lmg_tune_range("sell_nt", &g_sell_nt, -1, 1),
    lmg_tune_list("sell_ju", &g_sell_ju, 0, 5, 7, 8, 10),
    kLmgTuneEnd,
};

extern "C" {

int lmg_sell_sweep(int mode, int64_t n, const int64_t *slice_base, const int32_t *slice_len, const int32_t *slice_cmin,
                   const int32_t *rowlen, const void *col, int colmode, const double *val, int32_t max_len,
                   const double *x, const double *b, double *out, double alpha, double beta, double *partials,
                   double *norm2, void *stream)
{
    return sell_sweep<double>(mode, n, slice_base, slice_len, slice_cmin, rowlen, col, colmode, val, max_len, x, b, out, alpha,
                              beta, partials, norm2, stream);
}

int lmg_sell_sweep_f32(int mode, int64_t n, const int64_t *slice_base, const int32_t *slice_len, const int32_t *slice_cmin,
                       const int32_t *rowlen, const void *col, int colmode, const float *val, int32_t max_len,
                       const double *x, const double *b, double *out, double alpha, double beta, double *partials,
                       double *norm2, void *stream)
{
    return sell_sweep<float>(mode, n, slice_base, slice_len, slice_cmin, rowlen, col, colmode, val, max_len, x, b, out, alpha,
                             beta, partials, norm2, stream);
}

int64_t lmg_block_partials_count(int64_t n, int k)
{
    // one row of k sums per workgroup of the block sweep (kSlicesPerBlock slices of 64 rows), at least one row
    const int64_t nslices = n > 0 ? (n + LMG_WAVE - 1) / LMG_WAVE : 0;
    const int64_t nblocks = (nslices + kSlicesPerBlock - 1) / kSlicesPerBlock;
    return (nblocks < 1 ? 1 : nblocks) * (int64_t)(k < 1 ? 1 : k);
}

int lmg_sell_sweep_block(int mode, int k, int64_t n, const int64_t *slice_base, const int32_t *slice_len,
                         const int32_t *slice_cmin, const int32_t *rowlen, const void *col, int colmode, const double *val,
                         int32_t max_len, const double *X, const double *B, double *Out, double alpha, double beta,
                         double *partials, double *norm2, void *stream)
{
    if (!block_width_ok(k)) return LMG_ERR_ARG;
    if (n < 0 || n >= INT32_MAX - 64 || (colmode != 0 && colmode != 1) || max_len < 0) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!slice_base || !slice_len || !rowlen || !col || !val || !X) return LMG_ERR_ARG;
    if (colmode == 0 && !slice_cmin) return LMG_ERR_ARG;
    if (lmg_check_sweep_args(mode, X, B, Out, partials, norm2) != LMG_OK) return LMG_ERR_ARG;
    if (!lmg_aligned16(X) || !lmg_aligned16(B) || !lmg_aligned16(Out)) return LMG_ERR_ALIGN;      // (null is aligned)
    SArgs a;
    a.n = (int)n;
    a.nslices = (int)((n + LMG_WAVE - 1) / LMG_WAVE);
    a.nblocks = (a.nslices + kSlicesPerBlock - 1) / kSlicesPerBlock;
    a.blocks_per_xcd = (a.nblocks + 7) / 8;
    a.slice_base = reinterpret_cast<const long long *>(slice_base);
    a.slice_len = slice_len;
    a.slice_cmin = slice_cmin;
    a.rowlen = rowlen;
    a.col = col;
    a.val = val;
    a.x = X;
    a.b = B;
    a.out = Out;
    a.alpha = alpha;
    a.beta = beta;
    a.partial = (mode == MODE_RESIDUAL) ? partials : nullptr;
    hipStream_t st = lmg_stream(stream);
    const bool nt = g_sell_nt == 1 || (g_sell_nt < 0 && (int64_t)a.n * max_len >= g_sell_nt_entries);     // launch()'s rule
    int rc;
    if (colmode == 0) {
        rc = mode == MODE_RESIDUAL ? launch_block_k<MODE_RESIDUAL, true>(a, k, nt, st)
           : mode == MODE_JACOBI ? launch_block_k<MODE_JACOBI, true>(a, k, nt, st) : launch_block_k<MODE_SPMV, true>(a, k, nt, st);
    } else {
        rc = mode == MODE_RESIDUAL ? launch_block_k<MODE_RESIDUAL, false>(a, k, nt, st)
           : mode == MODE_JACOBI ? launch_block_k<MODE_JACOBI, false>(a, k, nt, st) : launch_block_k<MODE_SPMV, false>(a, k, nt, st);
    }
    if (rc != LMG_OK) return rc;
    if (mode == MODE_RESIDUAL && partials) return lmg_reduce_partials_strided(partials, a.nblocks, k, norm2, st);
    return LMG_OK;
}

int lmg_sell_slice_info(int64_t n, const int32_t *rowptr, const int32_t *colidx, int32_t *slice_len, int32_t *cmin,
                        int32_t *cmax, void *stream)
{
    if (n < 0) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!rowptr || !slice_len || !cmin || !cmax) return LMG_ERR_ARG;
    const int64_t nslices = (n + LMG_WAVE - 1) / LMG_WAVE;
    const unsigned grid = (unsigned)((nslices + kSlicesPerBlock - 1) / kSlicesPerBlock);
    hipLaunchKernelGGL(sell_slice_info_kernel, dim3(grid), dim3(kBlock), 0, lmg_stream(stream), n, nslices, rowptr,
                       colidx, slice_len, cmin, cmax);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_sell_fill(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                  const int64_t *slice_base, const int32_t *slice_cmin, int colmode, void *col_out, double *val_out,
                  void *stream)
{
    return sell_fill<double>(n, rowptr, colidx, vals, slice_base, slice_cmin, colmode, col_out, val_out, nullptr, stream);
}

int lmg_sell_fill_f32(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                      const int64_t *slice_base, const int32_t *slice_cmin, int colmode, void *col_out, float *val_out,
                      int32_t *flag, void *stream)
{
    return sell_fill<float>(n, rowptr, colidx, vals, slice_base, slice_cmin, colmode, col_out, val_out, flag, stream);
}

}  // extern "C"
