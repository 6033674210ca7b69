// Fused Gram-Schmidt kernels of the Krylov solvers (learnmultigrid_amd/krylov.py): k dot products in one pass over w,
// and w -+= sum_j coef[j] V_j with the coefficients read from device memory and |w|^2 folded in.  Bandwidth-bound and
// deterministic: a fixed grid, one partial per workgroup and column, a second small launch for the final sums, no
// atomics.  A basis is a row-major block V[k][ldv], ldv >= n and even (every row 16-byte aligned); the elements
// n .. ldv-1 of a row and the rows >= k are never touched.
//
// Second half: conjugate gradients on a block of K right-hand sides (krylov.py block_pcg), blocks X[i * K + j] as in
// sell.hip's block sweeps.  K dot products in one pass with the element <-> lane map and the order of lmg_dot (vec.hip),
// and the two vector updates of an iteration with their coefficients divided on the device from per-column scalars, a
// per-column mask that freezes a converged column, and |r|^2 folded into the first of them.
//
// Third part: flexible GMRES on a block of K right-hand sides (krylov.py block_fgmres): the Gram-Schmidt kernels of the first
// half on a basis of interleaved blocks, column j with the bits of the single-vector kernels on a contiguous copy of that
// column, a count of basis vectors per column, and a per-column scaling that empties a column with a factor of 0.
#include "lmg_common.hpp"

namespace {

constexpr int kKryMaxVectors = 65;      // restart <= 64: the basis of one cycle has restart + 1 rows
constexpr int kKryGrid = 1024;          // workgroups of every launch = partials per column, whatever n and k are
constexpr int kKryChunk = 16;           // columns whose loads one lane keeps in flight (and sums in registers)

// partial[(j0 + c) * kKryGrid + blockIdx.x] = this workgroup's share of V_(j0+c) . w, j0 = blockIdx.y * kKryChunk.
// Lane t of workgroup g owns the element pairs g * 256 + t, + 1024 * 256, ...: one 16-byte load of w and one of every
// column per step.  Per column one accumulator per lane, the pair added .x then .y; the last element of an odd n goes
// to lane 0 of workgroup 0 after its pairs.  None of this depends on k or on the column's place in its chunk.
__global__ void __launch_bounds__(kLmgBlock) multi_dot_kernel(int64_t n, int k, const double *V, int64_t ldv, const double *w,
                                                              double *partial)
{
    __shared__ double s_red[kKryChunk][kLmgBlock / LMG_WAVE];
    const int j0 = (int)blockIdx.y * kKryChunk;
    const int kc = min(k - j0, kKryChunk);
    const double *Vc = V + (int64_t)j0 * ldv;
    double acc[kKryChunk];
#pragma unroll
    for (int c = 0; c < kKryChunk; ++c) acc[c] = 0.0;
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kLmgBlock;
    const double2 *w2 = reinterpret_cast<const double2 *>(w);
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n2; i += stride) {
        const double2 wv = w2[i];
        double2 vv[kKryChunk];
#pragma unroll
        for (int c = 0; c < kKryChunk; ++c) {
            if (c < kc) vv[c] = reinterpret_cast<const double2 *>(Vc + (int64_t)c * ldv)[i];
            else vv[c] = make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int c = 0; c < kKryChunk; ++c) {
            if (c < kc) {
                acc[c] += vv[c].x * wv.x;
                acc[c] += vv[c].y * wv.y;
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double wl = w[n - 1];
#pragma unroll
        for (int c = 0; c < kKryChunk; ++c)
            if (c < kc) acc[c] += Vc[(int64_t)c * ldv + (n - 1)] * wl;
    }
    const int lane = threadIdx.x & (LMG_WAVE - 1), wave = threadIdx.x / LMG_WAVE;
#pragma unroll
    for (int c = 0; c < kKryChunk; ++c) {
        if (c < kc) {
            const double s = lmg_wave_sum(acc[c]);
            if (lane == 0) s_red[c][wave] = s;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < kc) {
        double tot = 0.0;
#pragma unroll
        for (int wv = 0; wv < kLmgBlock / LMG_WAVE; ++wv) tot += s_red[threadIdx.x][wv];
        partial[(int64_t)(j0 + (int)threadIdx.x) * kKryGrid + blockIdx.x] = tot;
    }
}

// out[j] = sum of the kKryGrid partials of column j = blockIdx.x, in the order of lmg_block_sum<1024>
__global__ void __launch_bounds__(kKryGrid) multi_final_kernel(const double *partial, double *out)
{
    __shared__ double s_red[kKryGrid / LMG_WAVE];
    const double tot = lmg_block_sum<kKryGrid>(partial[(int64_t)blockIdx.x * kKryGrid + threadIdx.x], s_red);
    if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// w = w + (sign * coef[0]) * V_0, then + (sign * coef[1]) * V_1, ... for every element, j ascending, every product and
// every sum rounded on its own; sign = -1 is exactly w - coef[j] * V_j (negating is exact).  The same pair <-> lane map
// as multi_dot_kernel; the columns go through the registers kKryChunk at a time.  NORM: partial[blockIdx.x] = this
// workgroup's share of |w_new|^2.
template <bool NORM>
__global__ void __launch_bounds__(kLmgBlock) multi_axpy_kernel(int64_t n, int k, double sign, const double *V, int64_t ldv,
                                                               const double *coef, double *w, double *partial)
{
    __shared__ double s_coef[kKryMaxVectors];
    __shared__ double s_red[kLmgBlock / LMG_WAVE];
    for (int j = threadIdx.x; j < k; j += kLmgBlock) s_coef[j] = sign * coef[j];
    __syncthreads();
    double acc = 0.0;
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kLmgBlock;
    double2 *w2 = reinterpret_cast<double2 *>(w);
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n2; i += stride) {
        double2 wv = w2[i];
        for (int j0 = 0; j0 < k; j0 += kKryChunk) {
            const int kc = min(k - j0, kKryChunk);
            const double *Vc = V + (int64_t)j0 * ldv;
            double2 vv[kKryChunk];
#pragma unroll
            for (int c = 0; c < kKryChunk; ++c) {
                if (c < kc) vv[c] = reinterpret_cast<const double2 *>(Vc + (int64_t)c * ldv)[i];
                else vv[c] = make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int c = 0; c < kKryChunk; ++c) {
                if (c < kc) {
                    const double cj = s_coef[j0 + c];
                    wv.x = wv.x + cj * vv[c].x;
                    wv.y = wv.y + cj * vv[c].y;
                }
            }
        }
        w2[i] = wv;
        if (NORM) {
            acc += wv.x * wv.x;
            acc += wv.y * wv.y;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double wl = w[n - 1];
        for (int j = 0; j < k; ++j) wl = wl + s_coef[j] * V[(int64_t)j * ldv + (n - 1)];
        w[n - 1] = wl;
        if (NORM) acc += wl * wl;
    }
    if (NORM) {
        const double tot = lmg_block_sum<kLmgBlock>(acc, s_red);
        if (threadIdx.x == 0) partial[blockIdx.x] = tot;
    }
}

// what both entry points ask of a basis and its vector
int basis_check(int64_t n, int k, const double *V, int64_t ldv, const double *w)
{
    if (k > 0 && (!V || ldv < n || (ldv & 1))) return LMG_ERR_ARG;
    if (!w) return LMG_ERR_ARG;
    if ((k > 0 && !lmg_aligned16(V)) || !lmg_aligned16(w)) return LMG_ERR_ALIGN;
    return LMG_OK;
}

// ---- conjugate gradients on a block of K columns -------------------------------------------------------------------------
// One row <-> lane map for the three kernels, dot_kernel's (vec.hip): kKryGrid workgroups of 256 lanes, lane t of workgroup
// g owns the rows g * 256 + t, + 262144, ...; a lane reads the K values of its row of a block as K / 2 16-byte loads.
constexpr int64_t kBcgStride = (int64_t)kKryGrid * kLmgBlock;

template <int K>
__device__ __forceinline__ void bcg_load_row(const double *B, int64_t row, double (&v)[K])
{
    const d2 *b2 = reinterpret_cast<const d2 *>(B + row * K);
#pragma unroll
    for (int h = 0; h < K / 2; ++h) {
        const d2 t = b2[h];
        v[2 * h] = t.x;
        v[2 * h + 1] = t.y;
    }
}

// Row `row` of B <- v for the columns with on[j] (wave-uniform): a pair of columns as one 16-byte store where both are
// on, 8 bytes where one is, nothing where neither is -- the bytes of a column that is off are never written.
template <int K>
__device__ __forceinline__ void bcg_store_row(double *B, int64_t row, const double (&v)[K], const bool (&on)[K])
{
    double *b = B + row * K;
#pragma unroll
    for (int h = 0; h < K / 2; ++h) {
        if (on[2 * h] && on[2 * h + 1]) {
            d2 t;
            t.x = v[2 * h];
            t.y = v[2 * h + 1];
            reinterpret_cast<d2 *>(b)[h] = t;
        } else if (on[2 * h]) {
            b[2 * h] = v[2 * h];
        } else if (on[2 * h + 1]) {
            b[2 * h + 1] = v[2 * h + 1];
        }
    }
}

// partial[j * kKryGrid + blockIdx.x] = this workgroup's share of column j's sum, in lmg_block_sum<256>'s order (one LDS
// row per column: no reuse hazard between the K reductions)
template <int K>
__device__ __forceinline__ void bcg_write_partials(const double (&acc)[K], double (*s_red)[kLmgBlock / LMG_WAVE], double *partial)
{
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double tot = lmg_block_sum<kLmgBlock>(acc[j], s_red[j]);
        if (threadIdx.x == 0) partial[(int64_t)j * kKryGrid + blockIdx.x] = tot;
    }
}

// Column j: acc = acc + x * y over the lane's rows in ascending order -- dot_kernel's sum on a contiguous copy of column j.
template <int K>
__global__ void __launch_bounds__(kLmgBlock) block_dot_kernel(int64_t n, const double *X, const double *Y, double *partial)
{
    __shared__ double s_red[K][kLmgBlock / LMG_WAVE];
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n; i += kBcgStride) {
        double x[K], y[K];
        bcg_load_row<K>(X, i, x);
        bcg_load_row<K>(Y, i, y);
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] += x[j] * y[j];
    }
    bcg_write_partials<K>(acc, s_red, partial);
}

// out[j] = the kKryGrid partials of column j = blockIdx.x in dot_final_kernel's order (lmg_block_sum<1024>).  MASK, the
// launch behind block_cg_step_kernel: a column stays on only while its |r|^2 is above its threshold.  Column j's scalars
// are read and written by workgroup j alone.
template <bool MASK>
__global__ void __launch_bounds__(kKryGrid) block_final_kernel(const double *partial, double *out, const double *tol2, double *mask)
{
    __shared__ double s_red[kKryGrid / LMG_WAVE];
    const double tot = lmg_block_sum<kKryGrid>(partial[(int64_t)blockIdx.x * kKryGrid + threadIdx.x], s_red);
    if (threadIdx.x == 0) {
        out[blockIdx.x] = tot;
        if (MASK) mask[blockIdx.x] = (mask[blockIdx.x] != 0.0 && tot > tol2[blockIdx.x]) ? 1.0 : 0.0;
    }
}

// alpha_j = rz_j / pAp_j (0 where the column is off or pAp_j == 0: every lane of every workgroup does the same division),
// x = alpha p + x and r = (-alpha) ap + r with product and sum rounded on their own -- axpby_kernel's bits with beta = 1 --
// for the columns that are on; a column that is off is neither computed nor stored.  Every column, on or off, adds the
// squares of its r as it now stands to its partial: block_dot_kernel's sum of (R, R) after the update.
template <int K>
__global__ void __launch_bounds__(kLmgBlock) block_cg_step_kernel(int64_t n, const double *rz, const double *pAp, const double *mask,
                                                                  const double *P, const double *AP, double *X, double *R,
                                                                  double *partial)
{
    __shared__ double s_red[K][kLmgBlock / LMG_WAVE];
    double alpha[K], acc[K];
    bool on[K], any = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        on[j] = mask[j] != 0.0;
        const double d = pAp[j];
        alpha[j] = (on[j] && d != 0.0) ? rz[j] / d : 0.0;
        any = any || on[j];
        acc[j] = 0.0;
    }
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n; i += kBcgStride) {
        double r[K];
        bcg_load_row<K>(R, i, r);
        if (any) {
            double p[K], ap[K], x[K];
            bcg_load_row<K>(P, i, p);
            bcg_load_row<K>(AP, i, ap);
            bcg_load_row<K>(X, i, x);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (on[j]) {
                    x[j] = alpha[j] * p[j] + x[j];
                    r[j] = (-alpha[j]) * ap[j] + r[j];
                }
            }
            bcg_store_row<K>(X, i, x, on);
            bcg_store_row<K>(R, i, r, on);
        }
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] += r[j] * r[j];
    }
    bcg_write_partials<K>(acc, s_red, partial);
}

// beta_j = rz_new_j / rz_old_j, p = z + beta p for the columns that are on -- axpby_kernel's bits with alpha = 1, its
// beta == 0 case (p = z, p is not read) included; a column that is off is neither computed nor stored.
template <int K>
__global__ void __launch_bounds__(kLmgBlock) block_cg_direction_kernel(int64_t n, const double *rz_new, const double *rz_old,
                                                                       const double *mask, const double *Z, double *P)
{
    double beta[K];
    bool on[K], any = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        on[j] = mask[j] != 0.0;
        beta[j] = on[j] ? rz_new[j] / rz_old[j] : 0.0;
        any = any || on[j];
    }
    if (!any) return;
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n; i += kBcgStride) {
        double z[K], p[K];
        bcg_load_row<K>(Z, i, z);
        bcg_load_row<K>(P, i, p);
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (on[j]) p[j] = (beta[j] == 0.0) ? z[j] : z[j] + beta[j] * p[j];
        bcg_store_row<K>(P, i, p, on);
    }
}

inline bool bcg_width_ok(int k) { return k == 2 || k == 4 || k == 8; }

// f(std::integral_constant<int, K>) for the block width k (checked by the caller)
template <typename F>
int bcg_with_width(int k, F &&f)
{
    return k == 2 ? f(std::integral_constant<int, 2>{}) : k == 4 ? f(std::integral_constant<int, 4>{})
                                                                 : f(std::integral_constant<int, 8>{});
}

// ---- flexible GMRES on a block of K columns ------------------------------------------------------------------------------
// The Gram-Schmidt kernels of the first half on the interleaved layout: a block basis is nb blocks, block i at V + i * ldb,
// and column j of it does what multi_dot_kernel / multi_axpy_kernel do on a contiguous copy of that column.  The map is
// theirs: lane t of workgroup g owns the ROW pairs g * 256 + t, + 262144, ... -- the 2 K contiguous doubles of a row pair
// are K 16-byte loads --, one accumulator per (block, column) and lane, row 2 p before row 2 p + 1, the last row of an odd
// n to lane 0 of workgroup 0 after its pairs.
constexpr int kBgmDotAcc = 32;          // accumulators of one lane in block_multi_dot_kernel: blocks per chunk = 32 / K
constexpr int kBgmAxpyCols = 16;        // columns of basis blocks one lane keeps in flight in block_multi_axpy_kernel: 16 / K blocks

struct BgmCounts {
    int c[8];
};
struct BgmScales {
    double s[8];
};

// partial[((i0 + c) * K + j) * kKryGrid + blockIdx.x] = this workgroup's share of V_(i0+c)[:, j] . W[:, j], i0 = blockIdx.y
// * C: W's row pair stays in registers over the C blocks of the chunk.
template <int K>
__global__ void __launch_bounds__(kLmgBlock) block_multi_dot_kernel(int64_t n, int nb, const double *V, int64_t ldb, const double *W,
                                                                    double *partial)
{
    constexpr int C = kBgmDotAcc / K;
    __shared__ double s_red[C * K][kLmgBlock / LMG_WAVE];
    const int i0 = (int)blockIdx.y * C;
    const int nc = min(nb - i0, C);
    const double *Vc = V + (int64_t)i0 * ldb;
    double acc[C][K];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < K; ++j) acc[c][j] = 0.0;
    const int64_t n2 = n >> 1;
    for (int64_t p = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; p < n2; p += kBcgStride) {
        double w0[K], w1[K], v0[C][K], v1[C][K];
        bcg_load_row<K>(W, 2 * p, w0);
        bcg_load_row<K>(W, 2 * p + 1, w1);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (c < nc) {
                bcg_load_row<K>(Vc + (int64_t)c * ldb, 2 * p, v0[c]);
                bcg_load_row<K>(Vc + (int64_t)c * ldb, 2 * p + 1, v1[c]);
            } else {
#pragma unroll
                for (int j = 0; j < K; ++j) v0[c][j] = v1[c][j] = 0.0;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (c < nc) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    acc[c][j] += v0[c][j] * w0[j];
                    acc[c][j] += v1[c][j] * w1[j];
                }
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double w[K];
        bcg_load_row<K>(W, n - 1, w);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (c < nc) {
                double v[K];
                bcg_load_row<K>(Vc + (int64_t)c * ldb, n - 1, v);
#pragma unroll
                for (int j = 0; j < K; ++j) acc[c][j] += v[j] * w[j];
            }
        }
    }
    const int lane = threadIdx.x & (LMG_WAVE - 1), wave = threadIdx.x / LMG_WAVE;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (c < nc) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const double s = lmg_wave_sum(acc[c][j]);
                if (lane == 0) s_red[c * K + j][wave] = s;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nc * K) {
        double tot = 0.0;
#pragma unroll
        for (int wv = 0; wv < kLmgBlock / LMG_WAVE; ++wv) tot += s_red[threadIdx.x][wv];
        partial[((int64_t)i0 * K + (int)threadIdx.x) * kKryGrid + blockIdx.x] = tot;
    }
}

// Column j: w = w + (sign * coef[i * K + j]) * V_i[:, j] for i = 0 .. cnt.c[j] - 1 ascending, every product and every sum
// rounded on its own -- multi_axpy_kernel's loop with k = cnt.c[j] --, stored with bcg_store_row: a column with a count of
// 0 is neither computed nor stored.  maxc = the largest count: the loop bound, the per-column test is wave-uniform.  NORM:
// partial[j * kKryGrid + blockIdx.x] = this workgroup's share of |W[:, j]|^2 as it now stands, every column.
template <int K, bool NORM>
__global__ void __launch_bounds__(kLmgBlock) block_multi_axpy_kernel(int64_t n, BgmCounts cnt, int maxc, double sign, const double *V,
                                                                     int64_t ldb, const double *coef, double *W, double *partial)
{
    constexpr int C = kBgmAxpyCols / K;
    __shared__ double s_coef[kKryMaxVectors * K];
    __shared__ double s_red[K][kLmgBlock / LMG_WAVE];
    for (int t = threadIdx.x; t < maxc * K; t += kLmgBlock) s_coef[t] = sign * coef[t];
    __syncthreads();
    bool on[K];
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        on[j] = cnt.c[j] > 0;
        acc[j] = 0.0;
    }
    const int64_t n2 = n >> 1;
    for (int64_t p = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; p < n2; p += kBcgStride) {
        double w0[K], w1[K];
        bcg_load_row<K>(W, 2 * p, w0);
        bcg_load_row<K>(W, 2 * p + 1, w1);
        for (int i0 = 0; i0 < maxc; i0 += C) {
            const int nc = min(maxc - i0, C);
            const double *Vc = V + (int64_t)i0 * ldb;
            double v0[C][K], v1[C][K];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (c < nc) {
                    bcg_load_row<K>(Vc + (int64_t)c * ldb, 2 * p, v0[c]);
                    bcg_load_row<K>(Vc + (int64_t)c * ldb, 2 * p + 1, v1[c]);
                } else {
#pragma unroll
                    for (int j = 0; j < K; ++j) v0[c][j] = v1[c][j] = 0.0;
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (c < nc) {
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        if (i0 + c < cnt.c[j]) {
                            const double cj = s_coef[(i0 + c) * K + j];
                            w0[j] = w0[j] + cj * v0[c][j];
                            w1[j] = w1[j] + cj * v1[c][j];
                        }
                    }
                }
            }
        }
        bcg_store_row<K>(W, 2 * p, w0, on);
        bcg_store_row<K>(W, 2 * p + 1, w1, on);
        if (NORM) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                acc[j] += w0[j] * w0[j];
                acc[j] += w1[j] * w1[j];
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double w[K];
        bcg_load_row<K>(W, n - 1, w);
        for (int i = 0; i < maxc; ++i) {
            double v[K];
            bcg_load_row<K>(V + (int64_t)i * ldb, n - 1, v);
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (i < cnt.c[j]) w[j] = w[j] + s_coef[i * K + j] * v[j];
        }
        bcg_store_row<K>(W, n - 1, w, on);
        if (NORM) {
#pragma unroll
            for (int j = 0; j < K; ++j) acc[j] += w[j] * w[j];
        }
    }
    if (NORM) bcg_write_partials<K>(acc, s_red, partial);
}

// W[:, j] = sc.s[j] * W[:, j], one product per element (axpby_kernel with beta == 0); a scale of 0 stores +0.0 whatever
// the element held.
template <int K>
__global__ void __launch_bounds__(kLmgBlock) block_scale_kernel(int64_t n, BgmScales sc, double *W)
{
    const int64_t stride = (int64_t)gridDim.x * kLmgBlock;
    bool all[K];
#pragma unroll
    for (int j = 0; j < K; ++j) all[j] = true;
    for (int64_t i = (int64_t)blockIdx.x * kLmgBlock + threadIdx.x; i < n; i += stride) {
        double w[K];
        bcg_load_row<K>(W, i, w);
#pragma unroll
        for (int j = 0; j < K; ++j) w[j] = (sc.s[j] == 0.0) ? 0.0 : sc.s[j] * w[j];
        bcg_store_row<K>(W, i, w, all);
    }
}

// what the two Gram-Schmidt entry points ask of a block basis of nb blocks and its block W
int block_basis_check(int k, int64_t n, int nb, const double *V, int64_t ldb, const double *W)
{
    if (nb > 0 && (!V || ldb < n * k || (ldb & 1))) return LMG_ERR_ARG;
    if (!W) return LMG_ERR_ARG;
    if ((nb > 0 && !lmg_aligned16(V)) || !lmg_aligned16(W)) return LMG_ERR_ALIGN;
    return LMG_OK;
}

}  // namespace

extern "C" {

int lmg_krylov_max_vectors(void) { return kKryMaxVectors; }

int64_t lmg_multi_partials_count(int64_t n, int k)
{
    (void)n;                                   // fixed geometry: kKryGrid partials per column for every n
    return (int64_t)kKryGrid * (k > 1 ? k : 1);
}

int lmg_multi_dot(int64_t n, int k, const double *d_V, int64_t ldv, const double *d_w, double *d_partials, double *d_out,
                  void *stream)
{
    if (n < 0 || k < 0 || k > kKryMaxVectors) return LMG_ERR_ARG;
    if (k == 0) return LMG_OK;
    if (!d_partials || !d_out) return LMG_ERR_ARG;
    if (n == 0) {
        if (hipMemsetAsync(d_out, 0, (size_t)k * sizeof(double), lmg_stream(stream)) != hipSuccess) return LMG_ERR_LAUNCH;
        return LMG_OK;
    }
    const int bad = basis_check(n, k, d_V, ldv, d_w);
    if (bad) return bad;
    const unsigned chunks = (unsigned)((k + kKryChunk - 1) / kKryChunk);
    hipLaunchKernelGGL(multi_dot_kernel, dim3(kKryGrid, chunks), dim3(kLmgBlock), 0, lmg_stream(stream), n, k, d_V, ldv, d_w,
                       d_partials);
    LMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(multi_final_kernel, dim3((unsigned)k), dim3(kKryGrid), 0, lmg_stream(stream), d_partials, d_out);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_multi_axpy(int64_t n, int k, int subtract, const double *d_V, int64_t ldv, const double *d_coef, double *d_w,
                   double *d_partials, double *d_norm2, void *stream)
{
    if (n < 0 || k < 0 || k > kKryMaxVectors) return LMG_ERR_ARG;
    if (d_norm2 && !d_partials) return LMG_ERR_ARG;
    if (k > 0 && !d_coef) return LMG_ERR_ARG;
    if (n == 0) {
        if (d_norm2 && hipMemsetAsync(d_norm2, 0, sizeof(double), lmg_stream(stream)) != hipSuccess) return LMG_ERR_LAUNCH;
        return LMG_OK;
    }
    if (k == 0 && !d_norm2) return LMG_OK;
    const int bad = basis_check(n, k, d_V, ldv, d_w);
    if (bad) return bad;
    const double sign = subtract ? -1.0 : 1.0;
    if (d_norm2) {
        hipLaunchKernelGGL(multi_axpy_kernel<true>, dim3(kKryGrid), dim3(kLmgBlock), 0, lmg_stream(stream), n, k, sign, d_V, ldv,
                           d_coef, d_w, d_partials);
        LMG_CHECK_LAUNCH();
        hipLaunchKernelGGL(multi_final_kernel, dim3(1), dim3(kKryGrid), 0, lmg_stream(stream), d_partials, d_norm2);
        LMG_CHECK_LAUNCH();
    } else {
        hipLaunchKernelGGL(multi_axpy_kernel<false>, dim3(kKryGrid), dim3(kLmgBlock), 0, lmg_stream(stream), n, k, sign, d_V, ldv,
                           d_coef, d_w, (double *)nullptr);
        LMG_CHECK_LAUNCH();
    }
    return LMG_OK;
}

int64_t lmg_block_dot_partials_count(int64_t n, int k)
{
    (void)n;                                   // fixed geometry: kKryGrid partials per column for every n
    return (int64_t)kKryGrid * (k > 1 ? k : 1);
}

int lmg_block_dot(int k, int64_t n, const double *d_X, const double *d_Y, double *d_partials, double *d_out, void *stream)
{
    if (!bcg_width_ok(k) || n < 0) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!d_X || !d_Y || !d_partials || !d_out) return LMG_ERR_ARG;
    if (!lmg_aligned16(d_X) || !lmg_aligned16(d_Y)) return LMG_ERR_ALIGN;
    hipStream_t st = lmg_stream(stream);
    const int rc = bcg_with_width(k, [&](auto kc) -> int {
        hipLaunchKernelGGL(block_dot_kernel<LMG_CT(kc)>, dim3(kKryGrid), dim3(kLmgBlock), 0, st, n, d_X, d_Y, d_partials);
        LMG_CHECK_LAUNCH();
        return LMG_OK;
    });
    if (rc != LMG_OK) return rc;
    hipLaunchKernelGGL(block_final_kernel<false>, dim3((unsigned)k), dim3(kKryGrid), 0, st, d_partials, d_out,
                       (const double *)nullptr, (double *)nullptr);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_block_cg_step(int k, int64_t n, const double *d_rz, const double *d_pAp, const double *d_tol2, double *d_mask,
                      const double *d_P, const double *d_AP, double *d_X, double *d_R, double *d_partials, double *d_rr,
                      void *stream)
{
    if (!bcg_width_ok(k) || n < 0) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!d_rz || !d_pAp || !d_tol2 || !d_mask || !d_P || !d_AP || !d_X || !d_R || !d_partials || !d_rr) return LMG_ERR_ARG;
    // in / out blocks of one update, and the two blocks that are written, must be different arrays
    if (d_X == d_P || d_R == d_AP || d_X == d_R || d_X == d_AP || d_R == d_P) return LMG_ERR_ARG;
    // the scalars the update reads are not the ones the launch behind it writes (d_mask is: by then every workgroup has read it)
    if (d_rr == d_rz || d_rr == d_pAp || d_rr == d_tol2 || d_rr == d_mask) return LMG_ERR_ARG;
    if (!lmg_aligned16(d_P) || !lmg_aligned16(d_AP) || !lmg_aligned16(d_X) || !lmg_aligned16(d_R)) return LMG_ERR_ALIGN;
    hipStream_t st = lmg_stream(stream);
    const int rc = bcg_with_width(k, [&](auto kc) -> int {
        hipLaunchKernelGGL(block_cg_step_kernel<LMG_CT(kc)>, dim3(kKryGrid), dim3(kLmgBlock), 0, st, n, d_rz, d_pAp,
                           (const double *)d_mask, d_P, d_AP, d_X, d_R, d_partials);
        LMG_CHECK_LAUNCH();
        return LMG_OK;
    });
    if (rc != LMG_OK) return rc;
    hipLaunchKernelGGL(block_final_kernel<true>, dim3((unsigned)k), dim3(kKryGrid), 0, st, d_partials, d_rr, d_tol2, d_mask);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_block_cg_direction(int k, int64_t n, const double *d_rz_new, const double *d_rz_old, const double *d_mask,
                           const double *d_Z, double *d_P, void *stream)
{
    if (!bcg_width_ok(k) || n < 0) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!d_rz_new || !d_rz_old || !d_mask || !d_Z || !d_P) return LMG_ERR_ARG;
    if (d_rz_new == d_rz_old || d_P == d_Z) return LMG_ERR_ARG;
    if (!lmg_aligned16(d_Z) || !lmg_aligned16(d_P)) return LMG_ERR_ALIGN;
    return bcg_with_width(k, [&](auto kc) -> int {
        hipLaunchKernelGGL(block_cg_direction_kernel<LMG_CT(kc)>, dim3(kKryGrid), dim3(kLmgBlock), 0, lmg_stream(stream), n,
                           d_rz_new, d_rz_old, d_mask, d_Z, d_P);
        LMG_CHECK_LAUNCH();
        return LMG_OK;
    });
}

int64_t lmg_block_multi_partials_count(int64_t n, int k, int nb)
{
    (void)n;                                   // fixed geometry: kKryGrid partials per block and column for every n
    return (int64_t)kKryGrid * (k > 1 ? k : 1) * (nb > 1 ? nb : 1);
}

int lmg_block_multi_dot(int k, int64_t n, int nb, const double *d_V, int64_t ldb, const double *d_W, double *d_partials,
                        double *d_out, void *stream)
{
    if (!bcg_width_ok(k) || n < 0 || nb < 0 || nb > kKryMaxVectors) return LMG_ERR_ARG;
    if (nb == 0) return LMG_OK;
    if (!d_partials || !d_out) return LMG_ERR_ARG;
    hipStream_t st = lmg_stream(stream);
    if (n == 0) {
        if (hipMemsetAsync(d_out, 0, (size_t)nb * k * sizeof(double), st) != hipSuccess) return LMG_ERR_LAUNCH;
        return LMG_OK;
    }
    const int bad = block_basis_check(k, n, nb, d_V, ldb, d_W);
    if (bad) return bad;
    const int rc = bcg_with_width(k, [&](auto kc) -> int {
        constexpr int C = kBgmDotAcc / LMG_CT(kc);
        hipLaunchKernelGGL(block_multi_dot_kernel<LMG_CT(kc)>, dim3(kKryGrid, (unsigned)((nb + C - 1) / C)), dim3(kLmgBlock), 0, st,
                           n, nb, d_V, ldb, d_W, d_partials);
        LMG_CHECK_LAUNCH();
        return LMG_OK;
    });
    if (rc != LMG_OK) return rc;
    hipLaunchKernelGGL(multi_final_kernel, dim3((unsigned)(nb * k)), dim3(kKryGrid), 0, st, d_partials, d_out);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_block_multi_axpy(int k, int64_t n, const int *h_counts, int subtract, const double *d_V, int64_t ldb, const double *d_coef,
                         double *d_W, double *d_partials, double *d_norm2, void *stream)
{
    if (!bcg_width_ok(k) || n < 0 || !h_counts) return LMG_ERR_ARG;
    BgmCounts cnt = {};
    int maxc = 0;
    for (int j = 0; j < k; ++j) {
        if (h_counts[j] < 0 || h_counts[j] > kKryMaxVectors) return LMG_ERR_ARG;
        cnt.c[j] = h_counts[j];
        if (h_counts[j] > maxc) maxc = h_counts[j];
    }
    if (d_norm2 && !d_partials) return LMG_ERR_ARG;
    if (maxc > 0 && !d_coef) return LMG_ERR_ARG;
    hipStream_t st = lmg_stream(stream);
    if (n == 0) {
        if (d_norm2 && hipMemsetAsync(d_norm2, 0, (size_t)k * sizeof(double), st) != hipSuccess) return LMG_ERR_LAUNCH;
        return LMG_OK;
    }
    if (maxc == 0 && !d_norm2) return LMG_OK;
    const int bad = block_basis_check(k, n, maxc, d_V, ldb, d_W);
    if (bad) return bad;
    const double sign = subtract ? -1.0 : 1.0;
    const int rc = bcg_with_width(k, [&](auto kc) -> int {
        if (d_norm2)
            hipLaunchKernelGGL((block_multi_axpy_kernel<LMG_CT(kc), true>), dim3(kKryGrid), dim3(kLmgBlock), 0, st, n, cnt, maxc, sign,
                               d_V, ldb, d_coef, d_W, d_partials);
        else
            hipLaunchKernelGGL((block_multi_axpy_kernel<LMG_CT(kc), false>), dim3(kKryGrid), dim3(kLmgBlock), 0, st, n, cnt, maxc, sign,
                               d_V, ldb, d_coef, d_W, (double *)nullptr);
        LMG_CHECK_LAUNCH();
        return LMG_OK;
    });
    if (rc != LMG_OK || !d_norm2) return rc;
    hipLaunchKernelGGL(block_final_kernel<false>, dim3((unsigned)k), dim3(kKryGrid), 0, st, d_partials, d_norm2,
                       (const double *)nullptr, (double *)nullptr);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_block_scale(int k, int64_t n, const double *h_scale, double *d_W, void *stream)
{
    if (!bcg_width_ok(k) || n < 0 || !h_scale) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!d_W) return LMG_ERR_ARG;
    if (!lmg_aligned16(d_W)) return LMG_ERR_ALIGN;
    BgmScales sc = {};
    for (int j = 0; j < k; ++j) sc.s[j] = h_scale[j];
    return bcg_with_width(k, [&](auto kc) -> int {
        hipLaunchKernelGGL(block_scale_kernel<LMG_CT(kc)>, dim3(lmg_grid_for(n, kLmgBlock)), dim3(kLmgBlock), 0, lmg_stream(stream), n,
                           sc, d_W);
        LMG_CHECK_LAUNCH();
        return LMG_OK;
    });
}

}  // extern "C"
