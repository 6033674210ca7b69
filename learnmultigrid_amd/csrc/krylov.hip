// Fused Gram-Schmidt kernels of the Krylov solvers (learnmultigrid_amd/krylov.py): k dot products in one pass over w,
// and w -+= sum_j coef[j] V_j with the coefficients read from device memory and |w|^2 folded in.  Bandwidth-bound and
// deterministic: a fixed grid, one partial per workgroup and column, a second small launch for the final sums, no
// atomics.  A basis is a row-major block V[k][ldv], ldv >= n and even (every row 16-byte aligned); the elements
// n .. ldv-1 of a row and the rows >= k are never touched.
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

}  // extern "C"
