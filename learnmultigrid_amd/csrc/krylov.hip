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

// ---- the two inner Krylov steps of a K-cycle visit -----------------------------------------------------------------------
// A step is: NP dot products of one vector p with NP vectors q in one pass, the coefficients from them, one vector update.
// The products are cut into G = kc_grid(n) shares whatever runs them: share g is what lane t = 0 .. 255 of "workgroup g"
// adds up over the element pairs g * 256 + t, + 256 G, ..., summed in lmg_block_sum<256>'s order.  Form 2 gives every share
// a workgroup of its own and a second launch that sums them; form 1 is one workgroup of 1024 lanes whose quarters take four
// shares at a time.  Both run the same three functions below, so no bit depends on the form.
constexpr int kKcShareElems = 2048;         // elements a share is sized for: four pair steps of 256 lanes
constexpr int kKcMaxGrid = 512;             // most shares; grid-stride beyond kKcShareElems * kKcMaxGrid elements
constexpr int kKcOneBlock = 1024;           // lanes of the one-launch form
constexpr int kKcQuarters = kKcOneBlock / kLmgBlock;
// Largest n that takes the one-launch form under form 0: the largest power of two at which it was no slower than two
// launches on an MI355X, replayed from a graph and launched eagerly (tools/time_kcycle.py steps; the table is in DESIGN.md
// section 3: from a graph one launch wins up to 4096 and loses from 8192, eagerly it wins up to 16384).
constexpr int64_t kKcOneLaunchMax = 1 << 12;

inline int kc_grid(int64_t n)
{
    int64_t g = (n + kKcShareElems - 1) / kKcShareElems;
    return (int)(g < 1 ? 1 : g > kKcMaxGrid ? kKcMaxGrid : g);
}

struct KcArgs {
    int64_t n;
    int G;
    const double *c1, *v1, *c2, *v2, *r;    // r: the right-hand side b (step 1), rt (step 2)
    double *out, *scal, *partial;           // out: rt (step 1), x_out (step 2)
};

template <int STEP>
struct KcStep {
    static constexpr int NP = STEP == 1 ? 2 : 3;
};

// acc[c] = lane t's part of share g of p . q_c.  Step 1: q = (b, v1), p = v1 (GCR) or c1; step 2: q = (v1, v2, rt), p = v2
// (GCR) or c2.  With GCR p is q_1 and is loaded once.
template <int STEP, bool GCR>
__device__ __forceinline__ void kc_lane_products(const KcArgs &a, int g, int t, double (&acc)[3])
{
    constexpr int NP = KcStep<STEP>::NP;
    const double *q[3] = {STEP == 1 ? a.r : a.v1, STEP == 1 ? a.v1 : a.v2, STEP == 1 ? nullptr : a.r};
    const double *p = STEP == 1 ? a.c1 : a.c2;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = 0.0;
    const int64_t n2 = a.n >> 1;
    const int64_t stride = (int64_t)a.G * kLmgBlock;
    for (int64_t i = (int64_t)g * kLmgBlock + t; i < n2; i += stride) {
        d2 qv[NP];
#pragma unroll
        for (int c = 0; c < NP; ++c) qv[c] = reinterpret_cast<const d2 *>(q[c])[i];
        const d2 pv = GCR ? qv[1] : reinterpret_cast<const d2 *>(p)[i];
#pragma unroll
        for (int c = 0; c < NP; ++c) {
            acc[c] += pv.x * qv[c].x;
            acc[c] += pv.y * qv[c].y;
        }
    }
    if ((a.n & 1) && g == 0 && t == 0) {
        const int64_t e = a.n - 1;
        double ql[NP];
#pragma unroll
        for (int c = 0; c < NP; ++c) ql[c] = q[c][e];
        const double pl = GCR ? ql[1] : p[e];
#pragma unroll
        for (int c = 0; c < NP; ++c) acc[c] += pl * ql[c];
    }
}

// tot[c] = product c from its G shares, in every lane of the workgroup: lane t < 256 adds share t and share t + 256 (0.0
// beyond G), 64-lane butterfly, the four waves in ascending order.  Lanes from 256 on (form 1) only keep the barriers.
template <int NP>
__device__ __forceinline__ void kc_totals(const double *share, int G, double (*s_red)[kLmgBlock / LMG_WAVE], double *s_tot,
                                          double (&tot)[3])
{
    const int t = threadIdx.x;
    if (t < kLmgBlock) {
        const int lane = t & (LMG_WAVE - 1), wave = t / LMG_WAVE;
#pragma unroll
        for (int c = 0; c < NP; ++c) {
            const double lo = t < G ? share[c * G + t] : 0.0;
            const double hi = t + kLmgBlock < G ? share[c * G + t + kLmgBlock] : 0.0;
            const double s = lmg_wave_sum(lo + hi);
            if (lane == 0) s_red[c][wave] = s;
        }
    }
    __syncthreads();
    if (t < NP) {
        double sum = 0.0;
#pragma unroll
        for (int w = 0; w < kLmgBlock / LMG_WAVE; ++w) sum += s_red[t][w];
        s_tot[t] = sum;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) tot[c] = c < NP ? s_tot[c] : 0.0;
}

// The coefficients from the products, in every lane alike, and the update of the pairs first, first + stride, ...; the
// writer (one lane of the launch) stores the scalars and the last element of an odd n.
template <int STEP>
__device__ __forceinline__ void kc_finish(const KcArgs &a, const double (&tot)[3], int64_t first, int64_t stride, bool writer)
{
    const int64_t n2 = a.n >> 1;
    d2 *out2 = reinterpret_cast<d2 *>(a.out);
    if (STEP == 1) {
        const double alpha1 = tot[0], rho1 = tot[1];
        const double t1 = rho1 != 0.0 ? alpha1 / rho1 : 0.0;
        if (writer) {
            a.scal[LMG_KC_ALPHA1] = alpha1;
            a.scal[LMG_KC_RHO1] = rho1;
            a.scal[LMG_KC_T1] = t1;
        }
        const double nt = -t1;
        for (int64_t i = first; i < n2; i += stride) {
            const d2 bv = reinterpret_cast<const d2 *>(a.r)[i], vv = reinterpret_cast<const d2 *>(a.v1)[i];
            d2 o;
            o.x = bv.x + nt * vv.x;
            o.y = bv.y + nt * vv.y;
            out2[i] = o;
        }
        if ((a.n & 1) && writer) a.out[a.n - 1] = a.r[a.n - 1] + nt * a.v1[a.n - 1];
    } else {
        const double gamma = tot[0], beta = tot[1], alpha2 = tot[2];
        const double rho1 = a.scal[LMG_KC_RHO1], t1 = a.scal[LMG_KC_T1];
        const double q = rho1 != 0.0 ? gamma / rho1 : 0.0;
        const double rho2 = beta - gamma * q;
        const double t2 = rho2 != 0.0 ? alpha2 / rho2 : 0.0;
        const double ca = t1 - q * t2;
        if (writer) {
            a.scal[LMG_KC_GAMMA] = gamma;
            a.scal[LMG_KC_BETA] = beta;
            a.scal[LMG_KC_ALPHA2] = alpha2;
            a.scal[LMG_KC_RHO2] = rho2;
            a.scal[LMG_KC_T2] = t2;
            a.scal[LMG_KC_A] = ca;
        }
        for (int64_t i = first; i < n2; i += stride) {
            const d2 x1 = reinterpret_cast<const d2 *>(a.c1)[i], x2 = reinterpret_cast<const d2 *>(a.c2)[i];
            d2 o;
            o.x = ca * x1.x + t2 * x2.x;
            o.y = ca * x1.y + t2 * x2.y;
            out2[i] = o;                    // (out may be c2: this lane has read its pair)
        }
        if ((a.n & 1) && writer) a.out[a.n - 1] = ca * a.c1[a.n - 1] + t2 * a.c2[a.n - 1];
    }
}

// form 2, first launch: workgroup g writes share g of every product to partial[c * G + g]
template <int STEP, bool GCR>
__global__ void __launch_bounds__(kLmgBlock) kc_shares_kernel(KcArgs a)
{
    constexpr int NP = KcStep<STEP>::NP;
    __shared__ double s_red[NP][kLmgBlock / LMG_WAVE];
    double acc[3];
    kc_lane_products<STEP, GCR>(a, (int)blockIdx.x, (int)threadIdx.x, acc);
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        const double tot = lmg_block_sum<kLmgBlock>(acc[c], s_red[c]);
        if (threadIdx.x == 0) a.partial[c * a.G + (int)blockIdx.x] = tot;
    }
}

// form 2, second launch: every workgroup sums the shares, forms the coefficients and updates the pairs of its share
template <int STEP>
__global__ void __launch_bounds__(kLmgBlock) kc_update_kernel(KcArgs a)
{
    constexpr int NP = KcStep<STEP>::NP;
    __shared__ double s_red[NP][kLmgBlock / LMG_WAVE];
    __shared__ double s_tot[NP];
    double tot[3];
    kc_totals<NP>(a.partial, a.G, s_red, s_tot, tot);
    kc_finish<STEP>(a, tot, (int64_t)blockIdx.x * kLmgBlock + threadIdx.x, (int64_t)a.G * kLmgBlock,
                    blockIdx.x == 0 && threadIdx.x == 0);
}

// form 1: one workgroup.  Quarter w (lanes 256 w .. 256 w + 255) is workgroup g0 + w of form 2 for g0 = 0, 4, ...; the
// shares stay in LDS.
template <int STEP, bool GCR>
__global__ void __launch_bounds__(kKcOneBlock) kc_one_kernel(KcArgs a)
{
    constexpr int NP = KcStep<STEP>::NP;
    __shared__ double s_share[NP * kKcMaxGrid];
    __shared__ double s_quarter[kKcQuarters][NP][kLmgBlock / LMG_WAVE];
    __shared__ double s_red[NP][kLmgBlock / LMG_WAVE];
    __shared__ double s_tot[NP];
    const int w = (int)threadIdx.x / kLmgBlock, t = (int)threadIdx.x % kLmgBlock;
    const int lane = t & (LMG_WAVE - 1), wave = t / LMG_WAVE;
    for (int g0 = 0; g0 < a.G; g0 += kKcQuarters) {
        const int g = g0 + w;
        if (g < a.G) {                      // (uniform over the waves of a quarter)
            double acc[3];
            kc_lane_products<STEP, GCR>(a, g, t, acc);
#pragma unroll
            for (int c = 0; c < NP; ++c) {
                const double s = lmg_wave_sum(acc[c]);
                if (lane == 0) s_quarter[w][c][wave] = s;
            }
        }
        __syncthreads();
        if (g < a.G && t < NP) {
            double tot = 0.0;
#pragma unroll
            for (int k = 0; k < kLmgBlock / LMG_WAVE; ++k) tot += s_quarter[w][t][k];
            s_share[t * a.G + g] = tot;
        }
        __syncthreads();
    }
    double tot[3];
    kc_totals<NP>(s_share, a.G, s_red, s_tot, tot);
    kc_finish<STEP>(a, tot, (int64_t)threadIdx.x, (int64_t)kKcOneBlock, threadIdx.x == 0);
}

template <int STEP>
int kc_launch(const KcArgs &a, bool gcr, int form, hipStream_t st)
{
    const bool one = form == 1 || (form == 0 && a.n <= kKcOneLaunchMax);
    if (one) {
        if (gcr) hipLaunchKernelGGL((kc_one_kernel<STEP, true>), dim3(1), dim3(kKcOneBlock), 0, st, a);
        else hipLaunchKernelGGL((kc_one_kernel<STEP, false>), dim3(1), dim3(kKcOneBlock), 0, st, a);
        LMG_CHECK_LAUNCH();
        return LMG_OK;
    }
    if (gcr) hipLaunchKernelGGL((kc_shares_kernel<STEP, true>), dim3((unsigned)a.G), dim3(kLmgBlock), 0, st, a);
    else hipLaunchKernelGGL((kc_shares_kernel<STEP, false>), dim3((unsigned)a.G), dim3(kLmgBlock), 0, st, a);
    LMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(kc_update_kernel<STEP>, dim3((unsigned)a.G), dim3(kLmgBlock), 0, st, a);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

}  // namespace

extern "C" {

int lmg_kcycle_grid(int64_t n) { return kc_grid(n); }

int64_t lmg_kcycle_partials_count(int64_t n) { return 3 * (int64_t)kc_grid(n); }

int64_t lmg_kcycle_one_launch_max(void) { return kKcOneLaunchMax; }

int lmg_kcycle_step1(int64_t n, int gcr, int form, const double *d_c1, const double *d_v1, const double *d_b, double *d_rt,
                     double *d_scal, double *d_partials, int64_t partials_count, void *stream)
{
    if (n < 1 || form < 0 || form > 2 || !d_c1 || !d_v1 || !d_b || !d_rt || !d_scal || !d_partials) return LMG_ERR_ARG;
    if (partials_count < lmg_kcycle_partials_count(n)) return LMG_ERR_ARG;
    if (d_rt == d_c1 || d_rt == d_v1 || d_rt == d_b) return LMG_ERR_ARG;
    if (!lmg_aligned16(d_c1) || !lmg_aligned16(d_v1) || !lmg_aligned16(d_b) || !lmg_aligned16(d_rt)) return LMG_ERR_ALIGN;
    const KcArgs a = {n, kc_grid(n), d_c1, d_v1, nullptr, nullptr, d_b, d_rt, d_scal, d_partials};
    return kc_launch<1>(a, gcr != 0, form, lmg_stream(stream));
}

int lmg_kcycle_step2(int64_t n, int gcr, int form, const double *d_c1, const double *d_v1, const double *d_c2,
                     const double *d_v2, const double *d_rt, double *d_scal, double *d_x_out, double *d_partials,
                     int64_t partials_count, void *stream)
{
    if (n < 1 || form < 0 || form > 2 || !d_c1 || !d_v1 || !d_c2 || !d_v2 || !d_rt || !d_scal || !d_x_out || !d_partials)
        return LMG_ERR_ARG;
    if (partials_count < lmg_kcycle_partials_count(n)) return LMG_ERR_ARG;
    if (d_x_out == d_c1 || d_x_out == d_v1 || d_x_out == d_v2 || d_x_out == d_rt) return LMG_ERR_ARG;
    if (!lmg_aligned16(d_c1) || !lmg_aligned16(d_v1) || !lmg_aligned16(d_c2) || !lmg_aligned16(d_v2) || !lmg_aligned16(d_rt) ||
        !lmg_aligned16(d_x_out))
        return LMG_ERR_ALIGN;
    const KcArgs a = {n, kc_grid(n), d_c1, d_v1, d_c2, d_v2, d_rt, d_x_out, d_scal, d_partials};
    return kc_launch<2>(a, gcr != 0, form, lmg_stream(stream));
}

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
