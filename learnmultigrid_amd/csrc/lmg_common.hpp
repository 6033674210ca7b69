// Shared helpers of the gfx950 kernels (wave64, 256 CUs in 8 XCDs): everything that more than one kernel file
// needs has its single definition here -- the grid of a grid-stride launch, the sweep modes and their argument rules, XCD-aware tile ownership and the
// persistent grid that goes with it, the fixed-order sums, the DPP lane shifts, and the 3x3 stencil view (slot masks,
// pattern-table limit).  The host half at the end is what sits between the C ABI and hipLaunchKernelGGL in more than
// one file: the rows of the tune-key tables, and the one body of a fused-pass entry point (argument groups, checks, dispatch).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "lmg.h"

#define LMG_WAVE 64

#define LMG_CHECK_LAUNCH()                                          \
    do {                                                            \
        hipError_t e__ = hipGetLastError();                         \
        if (e__ != hipSuccess) return LMG_ERR_LAUNCH;               \
    } while (0)

static inline hipStream_t lmg_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }
static inline bool lmg_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- launch geometry of the grid-stride kernels (vec.hip, dense.hip) -------------------------------------------------
constexpr int kLmgBlock = 256;
constexpr int kLmgMaxGrid = 256 * 8;   // 256 CUs x 8 resident workgroups: grid-stride beyond

static inline unsigned lmg_grid_for(int64_t n, int per_block)
{
    int64_t g = (n + per_block - 1) / per_block;
    if (g > kLmgMaxGrid) g = kLmgMaxGrid;
    if (g < 1) g = 1;
    return (unsigned)g;
}

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
// the strided form: norm2[j] = sum of partials[i * k + j], i < count, for j < k -- column j in lmg_reduce_partials' order
int lmg_reduce_partials_strided(const double *partials, int64_t count, int k, double *norm2, hipStream_t st);

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
// stencil_tile.hip, dia_tile.hip: two v_mov less per shift of a double); false is the plain old-value form that
// gs_wave.hip was built and measured with -- changing it there changes its generated code -- and the only correct one
// with a fill value other than 0.
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

// ---- census of the rows that do not hold the expected pattern (lmg_pattern_census, vec.hip) ------------------------
// A table of int32 over (line, cell of kLmgCensusCell columns) of a grid with `lines` lines of stride W, with a border
// of zeros in front: entry [y + 1][c + 1] of (lines + 1) x (cells + 1) is the number of such rows on the lines 0 .. y in
// the cells 0 .. c (2-D inclusive prefix sums), so any rectangle of cells is counted with four loads.  A cell counts the
// columns it has beyond the line end and the rows a short last line lacks as well: what is not there is not expected.
constexpr int kLmgCensusCell = 32;
__host__ __device__ inline int lmg_census_cells(int W) { return (W + kLmgCensusCell - 1) / kLmgCensusCell; }
__host__ __device__ inline int64_t lmg_census_count(int lines, int W) { return (int64_t)(lines + 1) * (lmg_census_cells(W) + 1); }
// Whether every row on the lines y0 .. y1, columns x0 .. x1 (all inclusive) holds the expected pattern: the one
// function the fused register pass and the host (lmg_stencil_smooth_uniform_items) decide with.  Conservative: the
// rectangle is widened to whole cells, and one that leaves the grid -- or a missing table -- answers no.
__host__ __device__ inline bool lmg_census_all_expected(const int32_t *table, int lines, int W, int y0, int y1, int x0, int x1)
{
    if (!table || y0 < 0 || y1 >= lines || y0 > y1 || x0 < 0 || x1 >= W || x0 > x1) return false;
    const int64_t cs = lmg_census_cells(W) + 1;
    const int ca = x0 / kLmgCensusCell, cb = x1 / kLmgCensusCell + 1;
    const int32_t *lo = table + (int64_t)y0 * cs, *hi = table + (int64_t)(y1 + 1) * cs;
    return hi[cb] - lo[cb] - hi[ca] + lo[ca] == 0;
}

// The loops that stage a pattern table (st_val, st_mask) into LDS stay in the kernels: handed to a helper, the table
// pointers are read from the kernel arguments at the call instead of inside the guarded loops, which reorders the
// scalar loads of every kernel of gs_wave.hip, stencil_tile.hip and stencil_fused.hip.

// =====================================================================================================================
// Host half
// =====================================================================================================================

// ---- tune keys (lmg_tune_set / lmg_tune_get, vec.hip) ---------------------------------------------------------------
// A file that owns knobs lists them once, next to the globals: the key, the int it sets, and the values it accepts --
// an inclusive range, or a short list of the only ones.
struct LmgTuneKey {
    const char *key;
    int *value;
    int lo, hi;             // accepted: lo .. hi, both included ...
    int nlist, list[6];     // ... or, with nlist > 0, exactly list[0 .. nlist)
};
constexpr LmgTuneKey lmg_tune_range(const char *key, int *value, int lo, int hi = INT_MAX)
{
    return {key, value, lo, hi, 0, {}};
}
template <typename... V>
constexpr LmgTuneKey lmg_tune_list(const char *key, int *value, V... v)
{
    return {key, value, 0, 0, (int)sizeof...(V), {v...}};
}
constexpr LmgTuneKey kLmgTuneEnd = {nullptr, nullptr, 0, 0, 0, {}};      // closes a table
// the tables, one per owning file (constant data: nothing registers itself when the library is loaded)
extern const LmgTuneKey lmg_tune_sweep[], lmg_tune_pcsr[], lmg_tune_rpat[], lmg_tune_stencil[], lmg_tune_fused[],
    lmg_tune_tile[], lmg_tune_dia[], lmg_tune_sell[], lmg_tune_gsw[], lmg_tune_gs[];

static inline const LmgTuneKey *lmg_tune_find(const LmgTuneKey *table, const char *key)
{
    for (; table->key; ++table)
        if (strcmp(table->key, key) == 0) return table;
    return nullptr;
}
static inline bool lmg_tune_accepts(const LmgTuneKey &k, int v)
{
    if (k.nlist == 0) return v >= k.lo && v <= k.hi;
    for (int i = 0; i < k.nlist; ++i)
        if (k.list[i] == v) return true;
    return false;
}

// ---- runtime sweep count / flag -> template argument ----------------------------------------------------------------
// f(std::integral_constant<int, S>) for S = sweeps in LO .. HI; any other count takes HI, like the `default:` of the
// switches this replaces (callers check the range first).  LMG_CT(s) reads the constant back inside the lambda.
template <int LO, int HI, typename F>
int lmg_with_sweeps(int sweeps, F &&f)
{
    if constexpr (LO < HI) {
        if (sweeps == LO) return f(std::integral_constant<int, LO>{});
        return lmg_with_sweeps<LO + 1, HI>(sweeps, f);
    } else {
        return f(std::integral_constant<int, HI>{});
    }
}
template <typename F>
int lmg_with_flag(bool flag, F &&f)
{
    return flag ? f(std::true_type{}) : f(std::false_type{});
}
// f(std::integral_constant<unsigned, M>) for the M of the list that union_mask equals; LMG_ERR_CAPACITY for a slot set
// outside the list: nothing is built for it, the caller runs the separate sweeps
template <unsigned... M, typename F>
int lmg_with_mask(uint32_t union_mask, F &&f)
{
    int rc = LMG_ERR_CAPACITY;
    (void)((union_mask == M && (rc = f(std::integral_constant<unsigned, M>{}), true)) || ...);
    return rc;
}
#define LMG_CT(c) decltype(c)::value

// ---- the fused smoothing passes: argument groups, their checks, and the one body of an entry point ------------------
// stencil_fused.hip (iterates in registers, MArgs) and stencil_tile.hip (iterates in LDS, TArgs) take the same
// arguments under the same rules; their argument structs name the shared fields alike, and each says in constexpr
// members where its rules differ:
//     kRowLimit            first row count refused
//     kOneRowIsCapacity    a single row answers LMG_ERR_CAPACITY
//     kProlMinCoarse, kProlStrideCovers, kProlChecksPairs      (prolongation, below)
//     kRestCoarseLimit                                         (restriction, below)
// The groups list their members in the order of the C ABI (include/lmg.h), so an entry point hands its own arguments
// on in braces.
struct LmgOperator {
    int64_t n;
    int32_t line_stride;
    const uint8_t *pid;
    int32_t npat;
    const double *st_val;
    const int32_t *st_mask;
    uint32_t union_mask;
    int32_t hot_pattern;
    const double *h_hot_val;
};
struct LmgSolve {           // a Chebyshev step: sweeps = its degree, omega = c_0
    int sweeps;
    const double *x_in, *b;
    double omega;
    double *x_out, *r_out;
};
struct LmgProl {
    int64_t n_coarse;
    int32_t coarse_stride;
    const double *e_coarse;
    const uint8_t *p_pid;
    int32_t p_npat;
    const double *p_val;
    const int32_t *p_mask;
    const int32_t *h_hot_pairs;
    const double *h_hot_pval;
};
struct LmgRest {
    int64_t n_coarse;
    int32_t coarse_stride;
    double *b_coarse;
    const uint8_t *r_pid;
    int32_t r_npat;
    const double *r_val;
    const int32_t *r_mask;
    int32_t hot_r;
    const double *h_hot_rval;
};

// a hot pattern the host can hand to a kernel in scalar registers: in the table, with values, and a diagonal to divide by
static inline bool lmg_hot_usable(int32_t hot_pattern, int32_t npat, const double *h_hot_val)
{
    return hot_pattern >= 0 && hot_pattern < npat && h_hot_val && h_hot_val[4] != 0.0;
}

// The operator, the vectors and the sweep count.  Returns 1 with everything in `a` set but the fields only one of the
// structs has (no transfer folded in), else the status to hand back: LMG_OK where there is nothing to do.
template <typename A>
int lmg_smooth_fill(A &a, const LmgOperator &op, const LmgSolve &v)
{
    const int64_t n = op.n;
    if (n < 0 || n >= A::kRowLimit || op.npat < 1 || op.npat > kMaxPat || (op.union_mask & ~kMask9)) return LMG_ERR_ARG;
    if (v.sweeps < 1 || v.sweeps > 3) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (A::kOneRowIsCapacity && n < 2) return LMG_ERR_CAPACITY;
    if (!op.pid || !op.st_val || !op.st_mask || !v.b || !v.x_out || v.x_in == v.x_out || v.r_out == v.x_out ||
        (v.r_out && v.r_out == v.x_in))
        return LMG_ERR_ARG;
    if (op.line_stride < 3 || op.line_stride > n) return LMG_ERR_ARG;
    a.n = (int)n;
    a.W = op.line_stride;
    a.lines = (int)((n + op.line_stride - 1) / op.line_stride);
    a.npat = op.npat;
    a.pid = op.pid;
    a.st_val = op.st_val;
    a.st_mask = op.st_mask;
    a.x = v.x_in;
    a.b = v.b;
    a.out = v.x_out;
    a.r = v.r_out;
    a.omega = v.omega;
    const bool hot = lmg_hot_usable(op.hot_pattern, op.npat, op.h_hot_val);
    a.hot = hot ? op.hot_pattern : -1;
    for (int k = 0; k < 9; ++k) a.hot_val[k] = hot ? op.h_hot_val[k] : 0.0;
    a.hot_rdiag = hot ? 1.0 / op.h_hot_val[4] : 0.0;
    a.ec = nullptr;
    a.nc = a.Wc = 0;
    a.ppid = nullptr;
    a.pp_val = nullptr;
    a.pp_mask = nullptr;
    a.pp_npat = 0;
    a.bc = nullptr;
    a.rpid = nullptr;
    a.rp_val = nullptr;
    a.rp_mask = nullptr;
    a.rp_npat = 0;
    a.phot[0] = a.phot[1] = a.rhot = -1;
    for (int k = 0; k < 9; ++k) a.phv[k] = a.rhv[k] = 0.0;
    return 1;
}

// The prolongation folded into a pass (x_in + P e_coarse).  Checked before the operator; set after it.
//     kProlMinCoarse       fewest coarse rows: 1 in the register pass, 2 in the tiled one (as found)
//     kProlStrideCovers    the coarse line stride must cover half the fine one: the register pass finds the 2 x 2 window
//                          of row (y, x) at ((y >> 1), (x >> 1)) from its lane number; not asked by the tiled pass (as found)
//     kProlChecksPairs     hot pair ids outside P's table are dropped (-1): tiled pass only; both kernels just compare
//                          the ids with the ones they load (as found)
template <typename A>
int lmg_prol_check(const LmgOperator &op, const LmgSolve &v, const LmgProl &p)
{
    if (!v.x_in || !p.e_coarse || !p.p_pid || !p.p_val || !p.p_mask || p.p_npat < 1 || p.p_npat > kMaxPat) return LMG_ERR_ARG;
    if (p.n_coarse < A::kProlMinCoarse || p.n_coarse >= (1ll << 31) || p.coarse_stride < 1 || p.coarse_stride > p.n_coarse)
        return LMG_ERR_ARG;
    if (p.e_coarse == v.x_out) return LMG_ERR_ARG;
    if (A::kProlStrideCovers && (int64_t)p.coarse_stride < ((int64_t)op.line_stride + 1) / 2) return LMG_ERR_ARG;
    return LMG_OK;
}
template <typename A>
void lmg_prol_set(A &a, const LmgProl &p)
{
    a.ec = p.e_coarse;
    a.nc = (int)p.n_coarse;
    a.Wc = p.coarse_stride;
    a.ppid = p.p_pid;
    a.pp_val = p.p_val;
    a.pp_mask = p.p_mask;
    a.pp_npat = p.p_npat;
    if (p.h_hot_pairs && p.h_hot_pval) {
        for (int k = 0; k < 2; ++k) {
            const int pair = p.h_hot_pairs[k];
            const bool ok = !A::kProlChecksPairs || (pair >= 0 && (pair & 0xff) < p.p_npat && (pair >> 8) < p.p_npat);
            a.phot[k] = ok ? pair : -1;
        }
        for (int k = 0; k < 9; ++k) a.phv[k] = p.h_hot_pval[k];
    }
}

// The restriction folded into a pass (b_coarse = R (b - A x_out)).  Checked before the operator; set after it.
//     kRestCoarseLimit     first coarse row count refused: 2^28 in the register pass, 2^31 in the tiled one (as found)
template <typename A>
int lmg_rest_check(const LmgOperator &op, const LmgSolve &v, const LmgRest &r)
{
    if (!r.b_coarse || !r.r_pid || !r.r_val || !r.r_mask || r.r_npat < 1 || r.r_npat > kMaxPat) return LMG_ERR_ARG;
    if (r.n_coarse < 1 || r.n_coarse >= A::kRestCoarseLimit || r.coarse_stride < 1 || r.coarse_stride > r.n_coarse)
        return LMG_ERR_ARG;
    if (r.b_coarse == v.x_in || r.b_coarse == v.x_out || r.b_coarse == v.b) return LMG_ERR_ARG;
    // row (Y, X) of R sits on the fine node (2 Y, 2 X): every such node of the fine grid must have its coarse row
    // -- and nothing else: the pass only writes b_coarse under those nodes, a larger coarse grid would keep stale rows
    const int64_t lines = op.n > 0 ? (op.n + op.line_stride - 1) / op.line_stride : 0;
    if ((int64_t)r.coarse_stride != ((int64_t)op.line_stride + 1) / 2 || (op.n % op.line_stride) != 0 ||
        r.n_coarse != ((lines + 1) / 2) * r.coarse_stride)
        return LMG_ERR_ARG;
    return LMG_OK;
}
template <typename A>
void lmg_rest_set(A &a, const LmgRest &r)
{
    a.bc = r.b_coarse;
    a.nc = (int)r.n_coarse;
    a.Wc = r.coarse_stride;
    a.rpid = r.r_pid;
    a.rp_val = r.r_val;
    a.rp_mask = r.r_mask;
    a.rp_npat = r.r_npat;
    if (r.hot_r >= 0 && r.hot_r < r.r_npat && r.h_hot_rval) {
        a.rhot = r.hot_r;
        for (int k = 0; k < 9; ++k) a.rhv[k] = r.h_hot_rval[k];
    }
}

// The body of every fused-pass entry point.  `a` arrives with the fields only its struct has; p / r: the transfer folded
// in, or null.  The transfers are checked first (prolongation, then restriction: a pass with both can also alias their
// coarse vectors), then the operator, where "nothing to do" answers; launch(a, m) runs with the slot set as
// std::integral_constant m, for the sets M.. the pass is built for.
template <unsigned... M, typename A, typename Launch>
int lmg_fused_pass(A a, const LmgOperator &op, const LmgSolve &v, const LmgProl *p, const LmgRest *r, Launch &&launch)
{
    int bad = p ? lmg_prol_check<A>(op, v, *p) : LMG_OK;
    if (!bad && r) bad = lmg_rest_check<A>(op, v, *r);
    if (bad) return bad;
    if (p && r && (const double *)r->b_coarse == p->e_coarse) return LMG_ERR_ARG;
    const int rc = lmg_smooth_fill(a, op, v);
    if (rc != 1) return rc;
    if (p) lmg_prol_set(a, *p);
    if (r) lmg_rest_set(a, *r);
    return lmg_with_mask<M...>(op.union_mask, [&](auto m) { return launch(a, m); });
}
