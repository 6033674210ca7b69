// Shared helpers of the gfx950 kernels (wave64, 256 CUs in 8 XCDs): everything that more than one kernel file
// needs has its single definition here -- the sweep modes and their argument rules, XCD-aware tile ownership and the
// persistent grid that goes with it, the fixed-order sums, the DPP lane shifts, and the 3x3 stencil view (slot masks,
// pattern-table limit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lmg.h"

#define LMG_WAVE 64

#define LMG_CHECK_LAUNCH()                                          \
    do {                                                            \
        hipError_t e__ = hipGetLastError();                         \
        if (e__ != hipSuccess) return LMG_ERR_LAUNCH;               \
    } while (0)

static inline hipStream_t lmg_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }
static inline bool lmg_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- the three sweeps every storage format offers (the `mode` of the lmg_*_sweep entry points) ---------------------
enum { MODE_RESIDUAL = 0, MODE_JACOBI = 1, MODE_SPMV = 2 };

// Which of b, out, partials, norm2 a mode needs; x != out because the sweeps are not in-place.  Whether x itself may be
// null differs between the formats (an empty matrix never reads it) and stays with the caller.
static inline int lmg_check_sweep_args(int mode, const double *x, const double *b, const double *out,
                                       const double *partials, const double *norm2)
{
    if (mode == MODE_SPMV) {
        if (!out || x == out) return LMG_ERR_ARG;
    } else if (mode == MODE_JACOBI) {
        if (!b || !out || x == out) return LMG_ERR_ARG;
    } else if (mode == MODE_RESIDUAL) {
        if (!b || (partials == nullptr) != (norm2 == nullptr) || (!out && !partials)) return LMG_ERR_ARG;
    } else {
        return LMG_ERR_ARG;
    }
    return LMG_OK;
}

// norm2[0] = sum of partials[0 .. count) in fixed order: the launch that follows a residual sweep (sweep.hip)
int lmg_reduce_partials(const double *partials, int64_t count, double *norm2, hipStream_t st);

// ---- XCD-aware tile ownership ---------------------------------------------------------------------------------------
// Workgroup b runs on XCD b % 8 (round-robin dispatch), so XCD k is given the k-th contiguous eighth of the tiles and
// its private 4 MiB L2 sees one sliding window of the vectors instead of eight interleaved ones.
// One tile per workgroup (grid = 8 * tiles_per_xcd); the caller drops tiles beyond the last.
__device__ __forceinline__ int lmg_xcd_tile(int tiles_per_xcd)
{
    return (int)(blockIdx.x & 7u) * tiles_per_xcd + (int)(blockIdx.x >> 3);
}
// Persistent workgroups: this one owns tiles first, first + stride, ... < end; first >= end: none at all.
struct LmgXcdTiles {
    int begin, end, first, stride;
};
__device__ __forceinline__ LmgXcdTiles lmg_xcd_tiles(int tiles, int tiles_per_xcd)
{
    LmgXcdTiles o;
    const int xcd = (int)(blockIdx.x & 7u), slot = (int)(blockIdx.x >> 3);
    o.stride = (int)(gridDim.x >> 3);
    o.begin = xcd * tiles_per_xcd;
    o.end = min(tiles, o.begin + tiles_per_xcd);
    o.first = o.begin + slot;
    return o;
}
// Grid of a persistent sweep: as many workgroups per CU as registers + LDS admit (at most max_per_cu, and at most
// tune_per_cu where that is > 0), a multiple of 8, never more than one workgroup per tile.
template <int BLOCK, typename Kernel>
static inline unsigned lmg_persistent_grid(Kernel kernel, size_t lds_bytes, int max_per_cu, int tune_per_cu,
                                           int tiles_per_xcd)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, BLOCK, lds_bytes) != hipSuccess || per_cu < 1)
        per_cu = 4;
    if (per_cu > max_per_cu) per_cu = max_per_cu;
    if (tune_per_cu > 0 && tune_per_cu < per_cu) per_cu = tune_per_cu;
    int64_t grid = 256 * (int64_t)per_cu;
    if (grid > (int64_t)tiles_per_xcd * 8) grid = (int64_t)tiles_per_xcd * 8;
    return (unsigned)grid;
}

// Sum over the 64 lanes of a wave, fixed butterfly order (deterministic).
__device__ __forceinline__ double lmg_wave_sum(double v)
{
#pragma unroll
    for (int off = LMG_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, LMG_WAVE);
    return v;
}

// Block-wide sum in fixed order; result valid in thread 0.  s_red holds BLOCK/64 doubles.
template <int BLOCK>
__device__ __forceinline__ double lmg_block_sum(double v, double *s_red)
{
    v = lmg_wave_sum(v);
    const int lane = threadIdx.x & (LMG_WAVE - 1), wave = threadIdx.x / LMG_WAVE;
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    double tot = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < BLOCK / LMG_WAVE; ++w) tot += s_red[w];
    }
    return tot;
}

// ---- DPP shifts of a double by one lane across the whole wave ------------------------------------------------------
// CTRL 0x138 (wave_shr:1): lane i <- lane i-1; 0x130 (wave_shl:1): lane i <- lane i+1.  The lane without a source
// (0 resp. 63) keeps `old`.  BOUND_CTRL is the caller's choice and stays visible at every call site: true makes the
// instruction itself write 0 to that lane, so no register has to be cleared for it first (stencil_fused.hip,
// dia_tile.hip); false is the plain old-value form that stencil_tile.hip and gs_wave.hip were built and measured
// with -- changing it there changes their generated code -- and the only correct one with a fill value other than 0.
template <int CTRL, bool BOUND_CTRL>
__device__ __forceinline__ double lmg_dpp_shift(double old, double src)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, 0xf, 0xf, BOUND_CTRL);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, 0xf, 0xf, BOUND_CTRL);
    return __hiloint2double(hi, lo);
}
template <bool BOUND_CTRL>
__device__ __forceinline__ double dpp_lower(double src)      // lane i <- lane i-1, lane 0 <- 0
{
    return lmg_dpp_shift<0x138, BOUND_CTRL>(0.0, src);
}
template <bool BOUND_CTRL>
__device__ __forceinline__ double dpp_upper(double src)      // lane i <- lane i+1, lane 63 <- 0
{
    return lmg_dpp_shift<0x130, BOUND_CTRL>(0.0, src);
}
// the same with a fill value for the end lane
__device__ __forceinline__ double dpp_from_lower_lane(double src, double lane0) { return lmg_dpp_shift<0x138, false>(lane0, src); }
__device__ __forceinline__ double dpp_from_upper_lane(double src, double lane63) { return lmg_dpp_shift<0x130, false>(lane63, src); }

typedef double d2 __attribute__((ext_vector_type(2)));
struct __attribute__((aligned(8))) d2u { double a, b; };      // 16 bytes at 8-byte alignment

// ---- the 3x3 stencil view of a row: entry at column - row = c*W + d, c, d in {-1, 0, 1}, is slot (c+1)*3 + (d+1) ----
constexpr int kMaxPat = 64;                   // stencil patterns held in LDS (9 values each)
constexpr unsigned kMask9 = 0x1FFu;           // full 3x3
constexpr unsigned kMask5 = 0x0BAu;           // {-W, -1, 0, +1, +W}
constexpr unsigned kMask1D = 0x038u;          // {-1, 0, +1}
constexpr unsigned kMask7a = 0x1BBu;          // 5-point + {-W-1, +W+1}: P1 on triangles cut along one diagonal
constexpr unsigned kMask7b = 0x0FEu;          // 5-point + {-W+1, +W-1}: the other diagonal
constexpr unsigned kMaskUpper = 0x007u;       // the line above
constexpr unsigned kMaskLower = 0x1C0u;       // the line below
constexpr unsigned kMaskCorners = 0x145u;     // slots 0, 2, 6, 8: the diagonal neighbours
constexpr unsigned kMaskOffLine = kMaskUpper | kMaskLower;      // 0x1C7: any slot that needs the line stride

// The loops that stage a pattern table (st_val, st_mask) into LDS stay in the kernels: handed to a helper, the table
// pointers are read from the kernel arguments at the call instead of inside the guarded loops, which reorders the
// scalar loads of every kernel of gs_wave.hip, stencil_tile.hip and stencil_fused.hip.
