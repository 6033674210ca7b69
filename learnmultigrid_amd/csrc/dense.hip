// Dense kernels of the coarsest-level solve (coarse.py): GEMV on rows, block diagonals and windows of a vector, the first
// and last product of the block solvers with their permutation folded in, and the setup helpers (CSR -> dense, strided
// block copy, batched inverse).  Every product sums a row through ONE routine, lmg_row_partial (the gather kernels through
// coarse_gather_rows), which is what makes the entry points of include/lmg.h agree bit for bit.  The GEMM is gemm.hip.
#include "lmg_common.hpp"

namespace {

// One wave per row, grid-stride over the rows: this wave takes the rows first, first + step, ...
struct WaveRows {
    int lane;
    int64_t first, step;
};
__device__ __forceinline__ WaveRows wave_rows()
{
    return {(int)(threadIdx.x & (LMG_WAVE - 1)), ((int64_t)blockIdx.x * kLmgBlock + threadIdx.x) / LMG_WAVE,
            (int64_t)gridDim.x * kLmgBlock / LMG_WAVE};
}

// A lane's share of the inner product of a row with x, `half` pairs long: the lane takes the pairs j = first, first + STEP,
// ... and adds M[2j] * x[2j], then M[2j+1] * x[2j+1].  CH = 1 waits for every load in turn; CH > 1 issues all loads of a
// chunk of CH pairs before its sums (a row of a few thousand entries is otherwise one memory latency per step) -- the
// same order of additions.  X16: x is 16-byte aligned and read like M; else two 8-byte loads per pair.
template <int CH, int STEP, bool X16>
__device__ __forceinline__ double lmg_row_partial(const double *Mr, const double *x, int64_t half, int first)
{
    const double2 *M2 = reinterpret_cast<const double2 *>(Mr);
    double s = 0.0;
    for (int64_t j0 = first; j0 < half; j0 += (int64_t)CH * STEP) {
        double2 mv[CH], xv[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int64_t j = j0 + (int64_t)c * STEP;
            const int64_t jj = j < half ? j : 0;
            mv[c] = M2[jj];
            if constexpr (X16) {
                xv[c] = reinterpret_cast<const double2 *>(x)[jj];
            } else {
                xv[c].x = x[2 * jj];
                xv[c].y = x[2 * jj + 1];
            }
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (j0 + (int64_t)c * STEP < half) {
                s += mv[c].x * xv[c].x;
                s += mv[c].y * xv[c].y;
            }
        }
    }
    return s;
}

// The two stores of a finished row sum (the library is built with -ffp-contract=off: an inlined helper rounds like the
// open-coded line): into row r of block k of a strided y, and through an index table with accumulate.
__device__ __forceinline__ void window_store(double *y0, int64_t ys, const double *z0, int64_t zs, double alpha, int64_t k,
                                             int64_t r, double s)
{
    y0[k * ys + r] = (z0 ? z0[k * zs + r] : 0.0) + alpha * s;
}
__device__ __forceinline__ void permuted_store(double *out, int d, double v, int accumulate)
{
    out[d] = accumulate ? v + out[d] : v;
}

// Dense y = M x, one wave per row, 16 bytes per lane per step, fixed summation order.
// HBM-bound: 8*n*m bytes of M per call.
// With bs > 0 the matrix is block diagonal, stored as n/bs dense bs x m blocks one after the
// other: row r multiplies the x segment of its block, x[(r/bs)*m .. +m).
__global__ void __launch_bounds__(kLmgBlock) dense_gemv_kernel(int64_t n, int64_t m, const double *M, const double *x0,
                                                               double *y, int64_t bs)
{
    const WaveRows w = wave_rows();
    const bool vec_ok = (m % 2 == 0);
    for (int64_t row = w.first; row < n; row += w.step) {
        const double *Mr = M + row * m;
        const double *x = bs > 0 ? x0 + (row / bs) * m : x0;
        double s = 0.0;
        if (vec_ok) {
            s = lmg_row_partial<1, LMG_WAVE, true>(Mr, x, m / 2, w.lane);
        } else {
            for (int64_t j = w.lane; j < m; j += LMG_WAVE) s += Mr[j] * x[j];
        }
        s = lmg_wave_sum(s);
        if (w.lane == 0) y[row] = s;
    }
}

// Y = M X on a block of K vectors (X[i * K + j]: row i, column j; K = 2, 4, 8): one wave per row like dense_gemv_kernel,
// M is read once for all K columns.  A lane takes the pairs (even m) or elements (odd m) dense_gemv_kernel gives it and
// adds them in lmg_row_partial's order, the wave butterfly runs per column: column j has the bits of dense_gemv_kernel
// on column j.  The two rows of X a pair multiplies are 2 K contiguous doubles, read as 16-byte loads.
template <int K>
__global__ void __launch_bounds__(kLmgBlock) dense_gemv_block_kernel(int64_t n, int64_t m, const double *M, const double *X,
                                                                     double *Y)
{
    const WaveRows w = wave_rows();
    const d2 *X2 = reinterpret_cast<const d2 *>(X);
    const bool vec_ok = (m % 2 == 0);
    for (int64_t row = w.first; row < n; row += w.step) {
        const double *Mr = M + row * m;
        double s[K];
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] = 0.0;
        if (vec_ok) {
            const double2 *M2 = reinterpret_cast<const double2 *>(Mr);
            for (int64_t j = w.lane; j < m / 2; j += LMG_WAVE) {
                const double2 mv = M2[j];
                d2 xa[K / 2], xb[K / 2];
#pragma unroll
                for (int h = 0; h < K / 2; ++h) {
                    xa[h] = X2[j * K + h];                      // row 2 j
                    xb[h] = X2[j * K + K / 2 + h];              // row 2 j + 1
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    s[k] += mv.x * xa[k / 2][k & 1];
                    s[k] += mv.y * xb[k / 2][k & 1];
                }
            }
        } else {
            for (int64_t j = w.lane; j < m; j += LMG_WAVE) {
                const double mv = Mr[j];
#pragma unroll
                for (int h = 0; h < K / 2; ++h) {
                    const d2 xv = X2[j * (K / 2) + h];
                    s[2 * h] += mv * xv[0];
                    s[2 * h + 1] += mv * xv[1];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] = lmg_wave_sum(s[k]);
        if (w.lane == 0) {
            d2 *Y2 = reinterpret_cast<d2 *>(Y) + row * (K / 2);
#pragma unroll
            for (int h = 0; h < K / 2; ++h) {
                d2 o;
                o[0] = s[2 * h];
                o[1] = s[2 * h + 1];
                Y2[h] = o;
            }
        }
    }
}

// The same product with one WORKGROUP (4 waves) per row: a few thousand long rows (the Schur-complement
// inverse of the banded coarse solver, 2967 x 2967) give one wave per row too little to keep 256 CUs busy
// (26 us for 70 MB; 4 waves per row: see DESIGN.md).  The four partial sums are added in wave order, so the
// result does not depend on the launch geometry of other rows -- but it differs in rounding from the
// one-wave kernel, which is why the choice between the two only depends on (n, m).
__global__ void __launch_bounds__(kLmgBlock) dense_gemv_wgrow_kernel(int64_t n, int64_t m, const double *M, const double *x,
                                                                     double *y)
{
    __shared__ double s_part[kLmgBlock / LMG_WAVE];
    const int t = threadIdx.x, lane = t & (LMG_WAVE - 1), w = t / LMG_WAVE;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        double s = lmg_row_partial<8, kLmgBlock, true>(M + row * m, x, m / 2, t);
        if ((m & 1) && t == 0) s += M[row * m + m - 1] * x[m - 1];
        s = lmg_wave_sum(s);
        if (lane == 0) s_part[w] = s;
        __syncthreads();
        if (t == 0) {
            double tot = 0.0;
#pragma unroll
            for (int q = 0; q < kLmgBlock / LMG_WAVE; ++q) tot += s_part[q];
            y[row] = tot;
        }
        __syncthreads();
    }
}

// Batched GEMV on windows of a vector: for block k and row r
//     y[k*ys + r] = (z ? z[k*zs + r] : 0) + alpha * sum_c M[k][r][c] * x[k*xs + c]
// (M: nb dense rows x cols blocks, row-major, one after the other).  One wave per row, like
// dense_gemv_kernel; the windows of neighbouring blocks may overlap (xs < cols).  This is the only
// kernel of the block-cyclic-reduction coarse solver (coarse.py BlockCyclicReduction).
__global__ void __launch_bounds__(kLmgBlock) dense_gemv_windows_kernel(int64_t nb, int64_t rows, int64_t cols, const double *M,
                                                                       const double *x0, int64_t xs, const double *z0, int64_t zs,
                                                                       double alpha, double *y0, int64_t ys)
{
    const WaveRows w = wave_rows();
    for (int64_t row = w.first; row < nb * rows; row += w.step) {
        const int64_t k = row / rows, r = row - k * rows;
        const double s = lmg_wave_sum(lmg_row_partial<1, LMG_WAVE, true>(M + row * cols, x0 + k * xs, cols / 2, w.lane));
        if (w.lane == 0) window_store(y0, ys, z0, zs, alpha, k, r, s);
    }
}

// The same with a table of window starts instead of a stride: x window of block k = x0[xoff[k] .. xoff[k] + cols)
// (the banded coarse solver's back-substitution x_I = y_I - (A_II^-1 A_IS) x_S: strip k couples to the separators on
// either side of it, which start at irregular offsets; 8-byte aligned windows are enough for the 16-byte loads of M).
__global__ void __launch_bounds__(kLmgBlock) dense_gemv_windows_off_kernel(int64_t nb, int64_t rows, int64_t cols, const double *M,
                                                                           const double *x0, const int *xoff, const double *z0,
                                                                           int64_t zs, double alpha, double *y0, int64_t ys)
{
    const WaveRows w = wave_rows();
    for (int64_t row = w.first; row < nb * rows; row += w.step) {
        const int64_t k = row / rows, r = row - k * rows;
        const double s = lmg_wave_sum(lmg_row_partial<1, LMG_WAVE, false>(M + row * cols, x0 + xoff[k], cols / 2, w.lane));
        if (w.lane == 0) window_store(y0, ys, z0, zs, alpha, k, r, s);
    }
}

// First and last product of the banded coarse solver with the permutation [strips | separators] folded in (no
// gather / scatter launches around the solve):
//   front: y = blockdiag(M) * b[perm[0 .. nI)]   and   tail_out[i] = b[perm[nI + i]]            (i < ntail)
//   back : out[perm[k*rows + r]] (+)= z[k*zs + r] + alpha * M_k[r,:] . x[xoff[k] ..)   and
//          out[perm[nI + i]] (+)= x[i]                                                          (i < ntail)
// The lane sums and reductions of dense_gemv_kernel / dense_gemv_windows_off_kernel, in deeper chunks.
__global__ void __launch_bounds__(kLmgBlock) coarse_front_kernel(int64_t n, int64_t bs, const double *M, const double *b,
                                                                 const int *perm, double *y, int64_t ntail, double *tail_out)
{
    const WaveRows w = wave_rows();
    for (int64_t row = w.first; row < n; row += w.step) {
        // a strip is a run of CONSECUTIVE unknowns (perm[k bs + c] = perm[k bs] + c: the caller's layout), so its
        // right-hand side is read in place
        const double *x = b + perm[(row / bs) * bs];
        const double s = lmg_wave_sum(lmg_row_partial<8, LMG_WAVE, false>(M + row * bs, x, bs / 2, w.lane));
        if (w.lane == 0) y[row] = s;
    }
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < ntail; i += (int64_t)gridDim.x * kLmgBlock)
        tail_out[i] = b[perm[n + i]];
}

__global__ void __launch_bounds__(kLmgBlock) coarse_back_kernel(int64_t nb, int64_t rows, int64_t cols, const double *M,
                                                                const double *x0, const int *xoff, const double *z0, int64_t zs,
                                                                double alpha, const int *perm, double *out, int accumulate,
                                                                int64_t ntail)
{
    const WaveRows w = wave_rows();
    for (int64_t row = w.first; row < nb * rows; row += w.step) {
        const int64_t k = row / rows, r = row - k * rows;
        const double s = lmg_wave_sum(lmg_row_partial<4, LMG_WAVE, false>(M + row * cols, x0 + xoff[k], cols / 2, w.lane));
        if (w.lane == 0) permuted_store(out, perm[row], z0[k * zs + r] + alpha * s, accumulate);
    }
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < ntail; i += (int64_t)gridDim.x * kLmgBlock)
        permuted_store(out, perm[nb * rows + i], x0[i], accumulate);
}

// The same two products for blocks that are NOT runs of consecutive unknowns (coarse.py GridBlockSolver: rectangular
// blocks of a grid, padded to one size): every operand index comes from a table,
//   front: y[k*bs + r] = sum_c M_k[r][c] * b[idx[k*bs + c]]  (idx < 0: padding, contributes 0),  tail_out[i] = b[tail_idx[i]]
//   back : out[oidx[k*rows + r]] (+)= z[k*zs + r] + alpha * sum_c M_k[r][c] * x[xidx[k*cols + c]]  (oidx < 0: padding row),
//          out[tail_idx[i]] (+)= x[i]
// (fixed order of additions: lane sums over 128-entry passes, butterfly over the wave)
constexpr int kCoarseRows = 36;       // rows of a block per workgroup: 9 per wave, all their loads in flight at once

// The body of both: one workgroup = kCoarseRows rows of ONE block (blockIdx.x; blockIdx.y: which rows).  The block's
// operand segment, element c = fill(k, c), is gathered ONCE into LDS (s_seg: cols doubles), then every wave walks its
// rows with all loads of all its rows issued before the first sum (rows are 50 - 300 entries: a wave per row with a
// grid-stride loop spent its time in three dependent round trips); store(k, r, sum) takes the row sums.  fill and store
// capture by VALUE: by reference the epilogue redoes its scalar address arithmetic row by row (40 - 100 instructions more).
template <typename Fill, typename Store>
__device__ __forceinline__ void coarse_gather_rows(int64_t rows, int64_t cols, const double *M, double *s_seg, Fill fill,
                                                   Store store)
{
    const int t = threadIdx.x, lane = t & (LMG_WAVE - 1), w = t / LMG_WAVE;
    const int64_t k = blockIdx.x, r0 = (int64_t)blockIdx.y * kCoarseRows;
    for (int64_t c = t; c < cols; c += kLmgBlock) s_seg[c] = fill(k, c);
    __syncthreads();
    const double2 *x2 = reinterpret_cast<const double2 *>(s_seg);
    constexpr int RPW = kCoarseRows / (kLmgBlock / LMG_WAVE);      // 9 rows per wave
    const int64_t half = cols / 2;
    double tot[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) tot[q] = 0.0;
    for (int64_t j0 = 0; j0 < half; j0 += LMG_WAVE) {              // (rows longer than 128 entries: another pass)
        const int64_t j = j0 + lane;
        double2 mv[RPW];
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            const int64_t r = r0 + w + 4 * q;
            mv[q] = (r < rows && j < half) ? reinterpret_cast<const double2 *>(M + (k * rows + r) * cols)[j] : double2{0.0, 0.0};
        }
        const double2 xv = j < half ? x2[j] : double2{0.0, 0.0};
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            double sacc = 0.0;
            sacc += mv[q].x * xv.x;
            sacc += mv[q].y * xv.y;
            tot[q] += lmg_wave_sum(sacc);
        }
    }
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const int64_t r = r0 + w + 4 * q;
        if (lane == 0 && r < rows) store(k, r, tot[q]);
    }
}

__global__ void __launch_bounds__(kLmgBlock) coarse_front_gather_kernel(int64_t nblocks, int64_t bs, const double *M,
                                                                        const double *b, const int *idx, double *y, int64_t ntail,
                                                                        const int *tail_idx, double *tail_out)
{
    extern __shared__ double s_seg[];                              // bs doubles
    coarse_gather_rows(
        bs, bs, M, s_seg,
        [=](int64_t k, int64_t c) {
            const int g = idx[k * bs + c];
            return g >= 0 ? b[g] : 0.0;
        },
        [=](int64_t k, int64_t r, double tot) { y[k * bs + r] = tot; });
    if (blockIdx.y == 0)
        for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < ntail; i += nblocks * kLmgBlock)
            tail_out[i] = b[tail_idx[i]];
}

__global__ void __launch_bounds__(kLmgBlock) coarse_back_gather_kernel(int64_t nb, int64_t rows, int64_t cols, const double *M,
                                                                       const double *x, const int *xidx, const double *z0,
                                                                       int64_t zs, double alpha, const int *oidx, double *out,
                                                                       int accumulate, int64_t ntail, const int *tail_idx)
{
    extern __shared__ double s_seg[];                              // cols doubles
    coarse_gather_rows(
        rows, cols, M, s_seg, [=](int64_t k, int64_t c) { return x[xidx[k * cols + c]]; },
        [=](int64_t k, int64_t r, double tot) {
            const int d = oidx[k * rows + r];
            if (d >= 0) permuted_store(out, d, z0[k * zs + r] + alpha * tot, accumulate);
        });
    if (blockIdx.y == 0)
        for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < ntail; i += nb * kLmgBlock)
            permuted_store(out, tail_idx[i], x[i], accumulate);
}

// dense[i][colidx[e]] += vals[e] for the entries e of row i (dense zero-initialised by the caller)
__global__ void __launch_bounds__(kLmgBlock) csr_to_dense_kernel(int64_t n, int64_t m, const int *rowptr, const int *colidx,
                                                                 const double *vals, double *dense)
{
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLmgBlock)
        for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) dense[i * m + colidx[e]] += vals[e];
}

// dst[k*ds + i] = src[k*ss + i], i < bs: strided copy of whole blocks
__global__ void __launch_bounds__(kLmgBlock) block_copy_kernel(int64_t nb, int64_t bs, const double *src, int64_t ss,
                                                               double *dst, int64_t ds)
{
    const int64_t total = nb * bs;
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kLmgBlock) {
        const int64_t k = i / bs, r = i - k * bs;
        dst[k * ds + r] = src[k * ss + r];
    }
}

// Batched inverse of small dense matrices (n <= 128): one workgroup per matrix, the matrix in LDS,
// in-place Gauss-Jordan with partial pivoting (row swaps recorded, undone as column swaps at the end).
// Setup-time helper of the coarse solvers (the leaves of coarse.py's block Schur recursion): replaces
// thousands of 25-50 us rocSOLVER getf2 panel launches -- and the 0.4 s it takes to load that library
// in a fresh process -- by one launch.  info[k] = 1 when a pivot of matrix k is exactly zero.
constexpr int kInvMax = 128;
__global__ void __launch_bounds__(kLmgBlock) batched_inverse_kernel(int n, const double *A, double *Ainv, int *info)
{
    extern __shared__ double s_a[];                  // n rows of stride n + 1
    __shared__ int s_piv[kInvMax];
    __shared__ int s_p;
    __shared__ double s_red_v[kLmgBlock / LMG_WAVE];
    __shared__ int s_red_i[kLmgBlock / LMG_WAVE];
    const int ld = n + 1, t = threadIdx.x;
    const double *Ak = A + (int64_t)blockIdx.x * n * n;
    for (int e = t; e < n * n; e += kLmgBlock) s_a[(e / n) * ld + e % n] = Ak[e];
    __syncthreads();
    bool singular = false;
    for (int k = 0; k < n; ++k) {
        // pivot: largest |a[i][k]|, i >= k (ties: smallest i)
        double best = -1.0;
        int bi = k;
        for (int i = k + t; i < n; i += kLmgBlock) {
            const double v = fabs(s_a[i * ld + k]);
            if (v > best) { best = v; bi = i; }
        }
#pragma unroll
        for (int off = LMG_WAVE / 2; off > 0; off >>= 1) {
            const double ov = __shfl_down(best, off, LMG_WAVE);
            const int oi = __shfl_down(bi, off, LMG_WAVE);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if ((t & (LMG_WAVE - 1)) == 0) { s_red_v[t / LMG_WAVE] = best; s_red_i[t / LMG_WAVE] = bi; }
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < kLmgBlock / LMG_WAVE; ++w)
                if (s_red_v[w] > best || (s_red_v[w] == best && s_red_i[w] < bi)) { best = s_red_v[w]; bi = s_red_i[w]; }
            s_p = bi;
            s_piv[k] = bi;
        }
        __syncthreads();
        const int p = s_p;
        if (p != k)
            for (int j = t; j < n; j += kLmgBlock) {
                const double tmp = s_a[k * ld + j];
                s_a[k * ld + j] = s_a[p * ld + j];
                s_a[p * ld + j] = tmp;
            }
        __syncthreads();
        const double piv = s_a[k * ld + k];
        if (piv == 0.0) { singular = true; break; }          // uniform: every thread reads the same LDS word
        __syncthreads();
        for (int j = t; j < n; j += kLmgBlock) s_a[k * ld + j] = (j == k ? 1.0 : s_a[k * ld + j]) / piv;
        __syncthreads();
        // eliminate column k from every other row; a[i][k] becomes -f * (1 / piv)
        for (int e = t; e < n * n; e += kLmgBlock) {
            const int i = e / n, j = e - i * n;
            if (i == k) continue;
            const double f = s_a[i * ld + k];
            if (j == k) continue;
            s_a[i * ld + j] -= f * s_a[k * ld + j];
        }
        __syncthreads();
        for (int i = t; i < n; i += kLmgBlock)
            if (i != k) s_a[i * ld + k] = -s_a[i * ld + k] * s_a[k * ld + k];
        __syncthreads();
    }
    if (singular) {
        if (t == 0) info[blockIdx.x] = 1;
        return;
    }
    for (int k = n - 1; k >= 0; --k) {               // undo the row swaps: swap COLUMNS k and piv[k]
        const int p = s_piv[k];
        if (p != k)
            for (int i = t; i < n; i += kLmgBlock) {
                const double tmp = s_a[i * ld + k];
                s_a[i * ld + k] = s_a[i * ld + p];
                s_a[i * ld + p] = tmp;
            }
        __syncthreads();
    }
    double *Ok = Ainv + (int64_t)blockIdx.x * n * n;
    for (int e = t; e < n * n; e += kLmgBlock) Ok[e] = s_a[(e / n) * ld + e % n];
    if (t == 0) info[blockIdx.x] = 0;
}

}  // namespace

extern "C" {

int lmg_dense_gemv(int64_t n, int64_t m, const double *M, const double *x, double *y, void *stream)
{
    if (n < 0 || m < 0 || (n > 0 && !y) || (n > 0 && m > 0 && (!M || !x))) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!lmg_aligned16(M) || !lmg_aligned16(x)) return LMG_ERR_ALIGN;
    if (n <= 8192 && m >= 1024) {
        hipLaunchKernelGGL(dense_gemv_wgrow_kernel, dim3((unsigned)(n < 4096 ? n : 4096)), dim3(kLmgBlock), 0,
                           lmg_stream(stream), n, m, M, x, y);
        LMG_CHECK_LAUNCH();
        return LMG_OK;
    }
    hipLaunchKernelGGL(dense_gemv_kernel, dim3(lmg_grid_for(n, kLmgBlock / LMG_WAVE)), dim3(kLmgBlock), 0,
                       lmg_stream(stream), n, m, M, x, y, (int64_t)0);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_dense_gemv_block(int k, int64_t n, int64_t m, const double *M, const double *X, double *Y, void *stream)
{
    if (k != 2 && k != 4 && k != 8) return LMG_ERR_ARG;
    if (n < 0 || m < 0) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!Y || (m > 0 && (!M || !X)) || X == Y) return LMG_ERR_ARG;
    if (!lmg_aligned16(M) || !lmg_aligned16(X) || !lmg_aligned16(Y)) return LMG_ERR_ALIGN;
    const dim3 grid(lmg_grid_for(n, kLmgBlock / LMG_WAVE)), block(kLmgBlock);
    hipStream_t st = lmg_stream(stream);
    if (k == 2) hipLaunchKernelGGL(dense_gemv_block_kernel<2>, grid, block, 0, st, n, m, M, X, Y);
    else if (k == 4) hipLaunchKernelGGL(dense_gemv_block_kernel<4>, grid, block, 0, st, n, m, M, X, Y);
    else hipLaunchKernelGGL(dense_gemv_block_kernel<8>, grid, block, 0, st, n, m, M, X, Y);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_dense_gemv_blockdiag(int64_t nblocks, int64_t bs, const double *M, const double *x, double *y,
                             void *stream)
{
    if (nblocks < 0 || bs < 0 || (nblocks * bs > 0 && (!M || !x || !y)) || x == y) return LMG_ERR_ARG;
    if (nblocks * bs == 0) return LMG_OK;
    if (!lmg_aligned16(M) || !lmg_aligned16(x) || (bs % 2)) return LMG_ERR_ALIGN;
    hipLaunchKernelGGL(dense_gemv_kernel, dim3(lmg_grid_for(nblocks * bs, kLmgBlock / LMG_WAVE)), dim3(kLmgBlock), 0,
                       lmg_stream(stream), nblocks * bs, bs, M, x, y, bs);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_dense_gemv_windows(int64_t nblocks, int64_t rows, int64_t cols, const double *M, const double *x,
                           int64_t x_stride, const double *z, int64_t z_stride, double alpha, double *y,
                           int64_t y_stride, void *stream)
{
    if (nblocks < 0 || rows < 0 || cols < 0 || x_stride < 0 || y_stride < rows || (z && z_stride < 0)) return LMG_ERR_ARG;
    if (nblocks * rows == 0) return LMG_OK;
    if (!M || !x || !y || x == y || z == y) return LMG_ERR_ARG;
    if (!lmg_aligned16(M) || !lmg_aligned16(x) || (cols % 2) || (x_stride % 2)) return LMG_ERR_ALIGN;
    hipLaunchKernelGGL(dense_gemv_windows_kernel, dim3(lmg_grid_for(nblocks * rows, kLmgBlock / LMG_WAVE)), dim3(kLmgBlock), 0,
                       lmg_stream(stream), nblocks, rows, cols, M, x, x_stride, z, z_stride, alpha, y, y_stride);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_dense_gemv_windows_off(int64_t nblocks, int64_t rows, int64_t cols, const double *M, const double *x,
                               const int32_t *x_offsets, const double *z, int64_t z_stride, double alpha, double *y,
                               int64_t y_stride, void *stream)
{
    if (nblocks < 0 || rows < 0 || cols < 0 || y_stride < rows || (z && z_stride < 0)) return LMG_ERR_ARG;
    if (nblocks * rows == 0) return LMG_OK;
    if (!M || !x || !x_offsets || !y || x == y) return LMG_ERR_ARG;
    if (!lmg_aligned16(M) || (cols % 2)) return LMG_ERR_ALIGN;
    hipLaunchKernelGGL(dense_gemv_windows_off_kernel, dim3(lmg_grid_for(nblocks * rows, kLmgBlock / LMG_WAVE)), dim3(kLmgBlock), 0,
                       lmg_stream(stream), nblocks, rows, cols, M, x, x_offsets, z, z_stride, alpha, y, y_stride);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_coarse_front(int64_t nblocks, int64_t bs, const double *M, const double *b, const int32_t *perm, double *y,
                     int64_t ntail, double *tail_out, void *stream)
{
    if (nblocks < 0 || bs < 0 || ntail < 0 || (nblocks * bs > 0 && (!M || !b || !perm || !y)) ||
        (ntail > 0 && (!tail_out || !b || !perm)) || b == y)
        return LMG_ERR_ARG;
    if (nblocks * bs == 0 && ntail == 0) return LMG_OK;
    if (!lmg_aligned16(M) || (bs % 2)) return LMG_ERR_ALIGN;
    hipLaunchKernelGGL(coarse_front_kernel, dim3(lmg_grid_for(nblocks * bs > 0 ? nblocks * bs : 1, kLmgBlock / LMG_WAVE)), dim3(kLmgBlock), 0,
                       lmg_stream(stream), nblocks * bs, bs, M, b, perm, y, ntail, tail_out);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_coarse_back(int64_t nblocks, int64_t rows, int64_t cols, const double *M, const double *x, const int32_t *x_offsets,
                    const double *z, int64_t z_stride, double alpha, const int32_t *perm, double *out, int accumulate,
                    int64_t ntail, void *stream)
{
    if (nblocks < 0 || rows < 0 || cols < 0 || ntail < 0 || z_stride < 0) return LMG_ERR_ARG;
    if (nblocks * rows == 0 && ntail == 0) return LMG_OK;
    if (!M || !x || !x_offsets || !z || !perm || !out || x == out || z == out) return LMG_ERR_ARG;
    if (!lmg_aligned16(M) || (cols % 2)) return LMG_ERR_ALIGN;
    hipLaunchKernelGGL(coarse_back_kernel, dim3(lmg_grid_for(nblocks * rows > 0 ? nblocks * rows : 1, kLmgBlock / LMG_WAVE)), dim3(kLmgBlock), 0,
                       lmg_stream(stream), nblocks, rows, cols, M, x, x_offsets, z, z_stride, alpha, perm, out, accumulate,
                       ntail);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_coarse_front_gather(int64_t nblocks, int64_t bs, const double *M, const double *b, const int32_t *idx, double *y,
                            int64_t ntail, const int32_t *tail_idx, double *tail_out, void *stream)
{
    if (nblocks < 0 || bs < 0 || ntail < 0 || (nblocks * bs > 0 && (!M || !b || !idx || !y)) ||
        (ntail > 0 && (!tail_out || !tail_idx || !b)) || b == y)
        return LMG_ERR_ARG;
    if (nblocks * bs == 0 && ntail == 0) return LMG_OK;
    if (!lmg_aligned16(M) || (bs % 2) || (reinterpret_cast<uintptr_t>(idx) & 7u)) return LMG_ERR_ALIGN;
    if (nblocks == 0 || bs == 0 || bs * 8 > 60000 || nblocks > 0x7fffffff) return LMG_ERR_CAPACITY;
    hipLaunchKernelGGL(coarse_front_gather_kernel, dim3((unsigned)nblocks, (unsigned)((bs + kCoarseRows - 1) / kCoarseRows)),
                       dim3(kLmgBlock), (size_t)bs * 8, lmg_stream(stream), nblocks, bs, M, b, idx, y, ntail, tail_idx, tail_out);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_coarse_back_gather(int64_t nblocks, int64_t rows, int64_t cols, const double *M, const double *x, const int32_t *xidx,
                           const double *z, int64_t z_stride, double alpha, const int32_t *oidx, double *out, int accumulate,
                           int64_t ntail, const int32_t *tail_idx, void *stream)
{
    if (nblocks < 0 || rows < 0 || cols < 0 || ntail < 0 || z_stride < 0) return LMG_ERR_ARG;
    if (nblocks * rows == 0 && ntail == 0) return LMG_OK;
    if (!M || !x || !xidx || !z || !oidx || !out || (ntail > 0 && !tail_idx) || x == out || z == out) return LMG_ERR_ARG;
    if (!lmg_aligned16(M) || (cols % 2) || (reinterpret_cast<uintptr_t>(xidx) & 7u)) return LMG_ERR_ALIGN;
    if (nblocks == 0 || rows == 0 || cols * 8 > 60000 || nblocks > 0x7fffffff) return LMG_ERR_CAPACITY;
    hipLaunchKernelGGL(coarse_back_gather_kernel, dim3((unsigned)nblocks, (unsigned)((rows + kCoarseRows - 1) / kCoarseRows)),
                       dim3(kLmgBlock), (size_t)cols * 8, lmg_stream(stream), nblocks, rows, cols, M, x, xidx, z, z_stride, alpha, oidx,
                       out, accumulate, ntail, tail_idx);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_csr_to_dense(int64_t n, int64_t m, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                     double *dense, void *stream)
{
    if (n < 0 || m < 0) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!rowptr || !colidx || !vals || !dense) return LMG_ERR_ARG;      // (rowptr[n] > 0 cannot be excluded on the host)
    hipLaunchKernelGGL(csr_to_dense_kernel, dim3(lmg_grid_for(n, kLmgBlock)), dim3(kLmgBlock), 0, lmg_stream(stream), n, m, rowptr,
                       colidx, vals, dense);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_batched_inverse(int64_t nmat, int32_t n, const double *A, double *Ainv, int32_t *info, void *stream)
{
    if (nmat < 0 || n < 1 || n > kInvMax) return LMG_ERR_ARG;
    if (nmat == 0) return LMG_OK;
    if (!A || !Ainv || !info || A == Ainv) return LMG_ERR_ARG;
    const size_t lds = (size_t)n * (n + 1) * sizeof(double);
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(batched_inverse_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kInvMax * (kInvMax + 1) * sizeof(double)));
    hipLaunchKernelGGL(batched_inverse_kernel, dim3((unsigned)nmat), dim3(kLmgBlock), lds, lmg_stream(stream), (int)n, A, Ainv,
                       info);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_block_copy(int64_t nblocks, int64_t bs, const double *src, int64_t src_stride, double *dst,
                   int64_t dst_stride, void *stream)
{
    if (nblocks < 0 || bs < 0 || src_stride < 0 || dst_stride < bs) return LMG_ERR_ARG;
    if (nblocks * bs == 0) return LMG_OK;
    if (!src || !dst) return LMG_ERR_ARG;
    hipLaunchKernelGGL(block_copy_kernel, dim3(lmg_grid_for(nblocks * bs, kLmgBlock)), dim3(kLmgBlock), 0, lmg_stream(stream),
                       nblocks, bs, src, src_stride, dst, dst_stride);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

}  // extern "C"
