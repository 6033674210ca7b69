// Multicolour Gauss-Seidel with everything on the device (ops.build_gs_schedule_device): a parallel greedy colouring of the
// pattern, a sliced-ELL copy of the matrix in colour order, and the sweep that walks it.  The rules: DESIGN.md section 3,
// "Multicolour Gauss-Seidel on the device"; the plain-Python restatement the kernels are compared with integer for integer
// and bit for bit: tests/color_ref.py.
//   - select:  G = the pattern of A and A^T without the diagonal.  Every uncoloured node whose key (hash(i), i) exceeds that
//              of every uncoloured neighbour is flagged: reads colours, writes its own flag;
//   - assign:  a flagged node takes the smallest colour none of its coloured neighbours has (a 64-bit mask in registers).  No
//              neighbour of a flagged node is flagged, so it reads colours no lane writes in that launch.  A node that would
//              need colour 64 reports its number with an atomic minimum on one 64-bit status word and stays uncoloured.  The
//              nodes left uncoloured are counted per workgroup (the host reads their sum, one count per round);
//   - twin count / fill / refill:  the colour classes as slices of 64 rows, every colour on a slice boundary (its last slice
//              filled up with empty rows, id -1), slice s padded to its longest row: entry j of scheduled row k at
//              slice_base[s] + 64 j + (k mod 64) as in sell.hip; a source index per entry refills the values;
//   - sweep:   one launch per colour, one wave per slice, lane = row: gs.hip's gs_update_row on coalesced streams.  The rows of
//              a colour read only other colours' x (and their own), so a launch has no race and its result does not depend
//              on the launch geometry; the backward sweep launches the colours in reverse.
// No LDS but the count of assign, no barrier but that one, no scratch.  Nothing waits for another workgroup.
#include "lmg_common.hpp"

namespace {

constexpr int kB = 256;
constexpr int kSlicesPerBlock = kB / LMG_WAVE;
constexpr int kMaxColors = LMG_COLOR_MAX;

__device__ __forceinline__ unsigned hash32(unsigned x)      // amg.hip's mixer
{
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// whether the key of an uncoloured neighbour j exceeds the key of i (then i is not flagged this round)
__device__ __forceinline__ bool beaten(int n, int i, unsigned hi, int j, const int *color)
{
    if (j == i || (unsigned)j >= (unsigned)n || color[j] >= 0) return false;
    const unsigned hj = hash32((unsigned)j);
    if (hi != hj) return hi < hj;
    return i < j;
}

__global__ void __launch_bounds__(kB) color_select_kernel(int n, const int *Ap, const int *Aj, const int *Tp, const int *Tj,
                                                          const int *color, int *flag)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    int f = 0;
    if (color[i] < 0) {
        const unsigned hi = hash32((unsigned)i);
        f = 1;
        for (int k = Ap[i]; f && k < Ap[i + 1]; ++k)
            if (beaten(n, i, hi, Aj[k], color)) f = 0;
        for (int k = Tp[i]; f && k < Tp[i + 1]; ++k)
            if (beaten(n, i, hi, Tj[k], color)) f = 0;
    }
    flag[i] = f;
}

__device__ __forceinline__ unsigned long long taken(int n, int i, int j, const int *color)
{
    if (j == i || (unsigned)j >= (unsigned)n) return 0ull;
    const int c = color[j];
    return c >= 0 ? 1ull << c : 0ull;
}

__global__ void __launch_bounds__(kB) color_assign_kernel(int n, const int *Ap, const int *Aj, const int *Tp, const int *Tj,
                                                          const int *flag, int *color, int *block_uncolored,
                                                          unsigned long long *status)
{
    __shared__ int s_red[kB / LMG_WAVE];
    const int i = blockIdx.x * kB + threadIdx.x;
    int left = 0;
    if (i < n) {
        int c = color[i];
        if (c < 0 && flag[i]) {
            unsigned long long mask = 0ull;
            for (int k = Ap[i]; k < Ap[i + 1]; ++k) mask |= taken(n, i, Aj[k], color);
            for (int k = Tp[i]; k < Tp[i + 1]; ++k) mask |= taken(n, i, Tj[k], color);
            if (~mask == 0ull) {
                atomicMin(status, (unsigned long long)i);
            } else {
                c = __ffsll((long long)~mask) - 1;
                color[i] = c;
            }
        }
        left = c < 0 ? 1 : 0;
    }
#pragma unroll
    for (int off = LMG_WAVE / 2; off > 0; off >>= 1) left += __shfl_down(left, off, LMG_WAVE);
    if ((threadIdx.x & (LMG_WAVE - 1)) == 0) s_red[threadIdx.x / LMG_WAVE] = left;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < kB / LMG_WAVE; ++w) tot += s_red[w];
        block_uncolored[blockIdx.x] = tot;
    }
}

// ---- the twin -----------------------------------------------------------------------------------------------------------
// one wave per slice: the row ids of the slice (-1 beyond the colour's last row), their lengths, the padded length
__global__ void __launch_bounds__(kB) twin_count_kernel(int nslices, int ncolors, const int *__restrict__ color_ptr,
                                                        const int *__restrict__ color_slice, const int *__restrict__ rows,
                                                        const int *__restrict__ rowptr, int *trow, int *tlen, int *slice_len)
{
    const int lane = threadIdx.x & (LMG_WAVE - 1);
    const int slice = blockIdx.x * kSlicesPerBlock + threadIdx.x / LMG_WAVE;
    if (slice >= nslices) return;
    // the colour c with color_slice[c] <= slice < color_slice[c + 1] (at most 64 colours, colours without rows have no slice)
    int lo = 0, hi = ncolors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (color_slice[mid] <= slice) lo = mid;
        else hi = mid - 1;
    }
    const int at = color_ptr[lo] + (slice - color_slice[lo]) * LMG_WAVE + lane;
    int row = -1, len = 0;
    if (at < color_ptr[lo + 1]) {
        row = rows[at];
        len = rowptr[row + 1] - rowptr[row];
    }
    const long long k = (long long)slice * LMG_WAVE + lane;
    trow[k] = row;
    tlen[k] = len;
#pragma unroll
    for (int off = LMG_WAVE / 2; off > 0; off >>= 1) {
        const int l2 = __shfl_down(len, off, LMG_WAVE);
        len = l2 > len ? l2 : len;
    }
    if (lane == 0) slice_len[slice] = len;
}

// lane = scheduled row: copies its entries to their padded positions, with where they came from
__global__ void __launch_bounds__(kB) twin_fill_kernel(int nslices, const int *__restrict__ trow, const int *__restrict__ rowptr,
                                                       const int *__restrict__ colidx, const double *__restrict__ vals,
                                                       const long long *__restrict__ slice_base, int *col, double *val, int *src)
{
    const int lane = threadIdx.x & (LMG_WAVE - 1);
    const int slice = blockIdx.x * kSlicesPerBlock + threadIdx.x / LMG_WAVE;
    if (slice >= nslices) return;
    const int row = trow[(long long)slice * LMG_WAVE + lane];
    if (row < 0) return;
    const int s = rowptr[row], e = rowptr[row + 1];
    const long long base = slice_base[slice] + lane;
    for (int k = s; k < e; ++k) {
        const long long p = base + (long long)(k - s) * LMG_WAVE;
        col[p] = colidx[k];
        val[p] = vals[k];
        src[p] = k;
    }
}

__global__ void __launch_bounds__(kB) twin_refill_kernel(long long padded, const int *__restrict__ src,
                                                         const double *__restrict__ vals, double *val)
{
    const long long p = (long long)blockIdx.x * kB + threadIdx.x;
    if (p >= padded) return;
    const int k = src[p];
    if (k >= 0) val[p] = vals[k];
}

// ---- the sweep ----------------------------------------------------------------------------------------------------------
struct CArgs {
    int slice0;                    // first slice of the colour
    int nslices;                   // its slices
    int nblocks;
    int blocks_per_xcd;
    const long long *slice_base;
    const int *slice_len;
    const int *trow;
    const int *tlen;
    const int *col;
    const double *val;
    double *x;
    const double *b;
};

// gs_update_row (gs.hip) on the twin: rsum over the entries off the diagonal in storage order with separately rounded
// products, diag = the last stored entry on it, x[row] = (b[row] - rsum) / diag unless diag == 0.  NT as in sell.hip.
template <int JU, bool NT>
__global__ void __launch_bounds__(kB) color_sweep_kernel(CArgs a)
{
    const int lane = threadIdx.x & (LMG_WAVE - 1), wave = threadIdx.x / LMG_WAVE;
    const int blk = lmg_xcd_tile(a.blocks_per_xcd);
    const int local = blk * kSlicesPerBlock + wave;
    if (blk >= a.nblocks || local >= a.nslices) return;
    const int slice = a.slice0 + local;
    const long long k = (long long)slice * LMG_WAVE + lane;
    const int row = a.trow[k];
    const int len = a.tlen[k];                                           // 0 for an empty lane
    const int slen = a.slice_len[slice];
    const long long base = a.slice_base[slice] + lane;
    const double bv = row >= 0 ? a.b[row] : 0.0;
    double rsum = 0.0, diag = 0.0;
    for (int j0 = 0; j0 < slen; j0 += JU) {
        int c[JU];
        double v[JU], xv[JU];
#pragma unroll
        for (int jj = 0; jj < JU; ++jj) {
            const int j = (j0 + jj < slen) ? j0 + jj : slen - 1;         // padded storage: always readable
            const long long e = base + (long long)j * LMG_WAVE;
            c[jj] = NT ? __builtin_nontemporal_load(a.col + e) : a.col[e];
            v[jj] = NT ? __builtin_nontemporal_load(a.val + e) : a.val[e];
        }
#pragma unroll
        for (int jj = 0; jj < JU; ++jj) xv[jj] = (j0 + jj < len) ? a.x[c[jj]] : 0.0;      // (an idle slot reads nothing)
#pragma unroll
        for (int jj = 0; jj < JU; ++jj) {
            const bool act = j0 + jj < len;
            const bool dg = c[jj] == row;
            const double s2 = rsum + v[jj] * xv[jj];
            rsum = (act && !dg) ? s2 : rsum;
            diag = (act && dg) ? v[jj] : diag;
        }
    }
    if (row >= 0 && diag != 0.0) a.x[row] = (bv - rsum) / diag;
}

// sell.hip's measured choices (launch()): nontemporal streams from 30 M padded entries, the unroll factor that leaves the
// fewest idle slots in the last trip over the longest row
constexpr int64_t kNtEntries = 30000000;

template <int JU>
void launch_color(const CArgs &a, bool nt, hipStream_t st)
{
    const dim3 grid((unsigned)(a.blocks_per_xcd * 8)), block(kB);
    if (nt) hipLaunchKernelGGL((color_sweep_kernel<JU, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((color_sweep_kernel<JU, false>), grid, block, 0, st, a);
}

inline int unroll_for(int max_len)
{
    if (max_len <= 12) return 4;
    int ju = 8, waste = (8 - max_len % 8) % 8;
    const int cand[2] = {7, 5};
    for (int k = 0; k < 2; ++k) {
        const int w = (cand[k] - max_len % cand[k]) % cand[k];
        if (w < waste) {
            waste = w;
            ju = cand[k];
        }
    }
    return ju;
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + kB - 1) / kB); }
inline bool rows_ok(int64_t n) { return n >= 0 && n < INT32_MAX - kB; }
inline unsigned slice_blocks(int64_t nslices) { return (unsigned)((nslices + kSlicesPerBlock - 1) / kSlicesPerBlock); }
inline bool slices_ok(int64_t nslices) { return nslices >= 0 && nslices < (INT32_MAX - kB) / LMG_WAVE; }

}  // namespace

extern "C" {

int lmg_color_select(int64_t n, const int32_t *rowptr, const int32_t *colidx, const int32_t *t_rowptr, const int32_t *t_colidx,
                     const int32_t *color, int32_t *flag, void *stream)
{
    if (!rows_ok(n) || !rowptr || !colidx || !t_rowptr || !t_colidx || !color || !flag) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    color_select_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, rowptr, colidx, t_rowptr, t_colidx, color, flag);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int64_t lmg_color_blocks(int64_t n) { return n > 0 ? (n + kB - 1) / kB : 0; }

int lmg_color_assign(int64_t n, const int32_t *rowptr, const int32_t *colidx, const int32_t *t_rowptr, const int32_t *t_colidx,
                     const int32_t *flag, int32_t *color, int32_t *block_uncolored, uint64_t *status, void *stream)
{
    if (!rows_ok(n) || !rowptr || !colidx || !t_rowptr || !t_colidx || !flag || !color || !block_uncolored || !status)
        return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    color_assign_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, rowptr, colidx, t_rowptr, t_colidx, flag, color,
                                                                  block_uncolored, (unsigned long long *)status);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_color_twin_count(int64_t nslices, int32_t ncolors, const int32_t *color_ptr, const int32_t *color_slice,
                         const int32_t *rows, const int32_t *rowptr, int32_t *twin_row, int32_t *twin_len, int32_t *slice_len,
                         void *stream)
{
    if (!slices_ok(nslices) || ncolors < 0 || ncolors > kMaxColors || !color_ptr || !color_slice || !rows || !rowptr ||
        !twin_row || !twin_len || !slice_len)
        return LMG_ERR_ARG;
    if (nslices == 0) return LMG_OK;
    if (ncolors == 0) return LMG_ERR_ARG;
    twin_count_kernel<<<slice_blocks(nslices), kB, 0, lmg_stream(stream)>>>((int)nslices, ncolors, color_ptr, color_slice, rows,
                                                                            rowptr, twin_row, twin_len, slice_len);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_color_twin_fill(int64_t nslices, const int32_t *twin_row, const int32_t *rowptr, const int32_t *colidx,
                        const double *vals, const int64_t *slice_base, int32_t *col, double *val, int32_t *src, void *stream)
{
    if (!slices_ok(nslices) || !twin_row || !rowptr || !colidx || !vals || !slice_base || !col || !val || !src)
        return LMG_ERR_ARG;
    if (nslices == 0) return LMG_OK;
    twin_fill_kernel<<<slice_blocks(nslices), kB, 0, lmg_stream(stream)>>>(
        (int)nslices, twin_row, rowptr, colidx, vals, reinterpret_cast<const long long *>(slice_base), col, val, src);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_color_twin_refill(int64_t padded, const int32_t *src, const double *vals, double *val, void *stream)
{
    if (padded < 0 || padded >= (int64_t)INT32_MAX * kB || !src || !vals || !val) return LMG_ERR_ARG;
    if (padded == 0) return LMG_OK;
    twin_refill_kernel<<<blocks(padded), kB, 0, lmg_stream(stream)>>>((long long)padded, src, vals, val);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_color_sweep(int32_t ncolors, const int32_t *h_color_slice, const int64_t *slice_base, const int32_t *slice_len,
                    const int32_t *twin_row, const int32_t *twin_len, const int32_t *col, const double *val, int32_t max_len,
                    int64_t padded, double *x, const double *b, int sweeps, int backward, void *stream)
{
    if (ncolors < 0 || ncolors > kMaxColors || sweeps < 0 || max_len < 0 || padded < 0 || (backward != 0 && backward != 1))
        return LMG_ERR_ARG;
    if (!h_color_slice || !slice_base || !slice_len || !twin_row || !twin_len || !col || !val || !x || !b) return LMG_ERR_ARG;
    for (int c = 0; c < ncolors; ++c)
        if (h_color_slice[c] < 0 || h_color_slice[c + 1] < h_color_slice[c]) return LMG_ERR_ARG;
    if (ncolors == 0 || sweeps == 0) return LMG_OK;
    hipStream_t st = lmg_stream(stream);
    const bool nt = padded >= kNtEntries;
    const int ju = unroll_for(max_len);
    CArgs a;
    a.slice_base = reinterpret_cast<const long long *>(slice_base);
    a.slice_len = slice_len;
    a.trow = twin_row;
    a.tlen = twin_len;
    a.col = col;
    a.val = val;
    a.x = x;
    a.b = b;
    for (int sw = 0; sw < sweeps; ++sw)
        for (int k = 0; k < ncolors; ++k) {
            const int c = backward ? ncolors - 1 - k : k;
            a.slice0 = h_color_slice[c];
            a.nslices = h_color_slice[c + 1] - h_color_slice[c];
            if (a.nslices == 0) continue;
            a.nblocks = (a.nslices + kSlicesPerBlock - 1) / kSlicesPerBlock;
            a.blocks_per_xcd = (a.nblocks + 7) / 8;
            if (ju == 4) launch_color<4>(a, nt, st);
            else if (ju == 5) launch_color<5>(a, nt, st);
            else if (ju == 7) launch_color<7>(a, nt, st);
            else launch_color<8>(a, nt, st);
        }
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

}  // extern "C"
