// Fused smoothing passes for SMALL grid-stencil levels (format of stencil.hip) for gfx950:
//     x_out = J^S(x_in)   [r = b - A x_out]          S = 1..3 weighted-Jacobi sweeps, x_in == NULL: zero iterate
// or, with CHEB, one Chebyshev smoothing step of degree S on D^-1 A (below) in place of the S Jacobi sweeps
// -- what stencil_fused.hip does for the multi-million-row levels, with the iterates in LDS instead of registers.
// On a level of 10^4 .. 10^6 rows a sweep is a 2 - 7 us launch (tools/time_small.py) and the register kernel is no
// help: a wave there walks 12 - 40 lines one after the other, 2 100 cycles each.  Here a WORKGROUP owns a tile of
// 64 columns x RR lines (its inner 64 - 2H x RR - 2H part is what it stores; H = S, +1 with the residual, -1 from a
// zero iterate), loads it once -- x, b, pattern ids --, runs the S sweeps between two LDS buffers with all four
// waves working on different lines of the same sweep, and stores the inner part: S (+1) launches become one, the
// dependent chain is S + 2 barriers long instead of S (+1) kernel boundaries.
// The arithmetic per row and sweep is the instruction sequence of stencil_sweep_kernel (slot order, separate
// multiply and add, omega * (rdiag * r)), so every value is bit-identical to the separate launches; as in
// stencil_fused.hip everything is a LINEAR index i = line * W + column, a column outside [0, W) being the linear
// neighbour in the adjacent line.
// The prologue REQUESTS, THEN CONSUMES: every global load a thread makes before the first barrier -- its lines of x, b and
// pattern ids, with a transfer the ids of P / R and the coarse windows, and its element of every table the workgroup
// stages -- is issued first, outside any branch, from an address that is valid whatever the element turns out to be
// (clamped indices; the diagonal of pattern i at i * 9 + 4 whatever its mask says); only behind the last of them does
// anything look at a result (the `ok` selects, the reciprocals, the hot-pattern tests, the LDS writes).  gfx950 counts
// loads in ONE in-order counter (vmcnt): written as `ok ? a.b[j] : 0.0` and as load-then-store staging loops, the
// prologue was a chain of seven dependent round trips per workgroup -- a wait per line, one per table loop, two in the
// reciprocal loop -- which a level of one or two workgroups per CU cannot hide; now it is one.  The same rule, for the
// same reason, governs the lines of stencil_fused.hip (see `struct Line` there).  What remains behind the wait: the row of
// P of an element without the usual pair (waves of the usual pair skip it), the tail of a table of more than
// kBlock / 9 patterns, and the further lines of the kernels that cannot hold all their lines' windows in 64 registers.
// (Tried: two columns per lane, 128-column tiles -- half the per-element overhead on paper, slower in practice: 9-point
// 2049^2 61.5 / 48.0 us against 49.6 / 41.4 us for 3 sweeps + residual / 3 sweeps; twice the LDS per tile, half the waves.)
#include "lmg_common.hpp"

namespace {

constexpr int kRB = 2;                        // consecutive lines of a tile a wave owns: a tile of RR lines is RR / 2 waves
                                              // (4 lines per wave: cfg#2 cycle 0.131 instead of 0.122 ms, cfg#4 equal)
constexpr int kCols = 64;                     // columns of a tile = lanes of a wave
constexpr int kLS = kCols + 2;                // LDS line stride: one guard column on either side

struct TArgs {
    // where this pass's argument rules differ from the register pass's (lmg_common.hpp)
    static constexpr int64_t kRowLimit = (1ll << 31) - 4096;     // rows are numbered in an int
    static constexpr bool kOneRowIsCapacity = false;             // (one row is shorter than any line stride: LMG_ERR_ARG)
    static constexpr int64_t kProlMinCoarse = 2;
    static constexpr bool kProlStrideCovers = false, kProlChecksPairs = true;
    static constexpr int64_t kRestCoarseLimit = 1ll << 31;
    int n, W, lines, npat;
    int tiles_x, tiles_y;
    const unsigned char *pid;
    const double *st_val;
    const int *st_mask;
    const double *x;          // may be NULL with ZERO
    const double *b;
    double *out;
    double *r;                // may be NULL without RESID
    double omega;
    int hot;
    double hot_val[9];
    double hot_rdiag;
    // PROL: the sweeps start from x + P e_c (Multigrid.py:115 folded into the post-smoothing pass), formed when the tile
    // is loaded: row i = y * W + x of P reads e_c at ((y >> 1) * Wc + (x >> 1)) + {0, 1, Wc, Wc + 1} (slots 0..3)
    const double *ec;
    int nc, Wc;
    const unsigned char *ppid;
    const double *pp_val;     // [pp_npat][4]
    const int *pp_mask;       // [pp_npat]
    int pp_npat;
    // REST: b_coarse = R (b - A x_out) instead of the residual (Multigrid.py:90 + :93 folded into the pre-smoothing pass):
    // row (Y, X) of R reads r at (2Y * W + 2X) + c * W + d, c, d in {-1, 0, 1} (slots 0..8); nc, Wc as above
    double *bc;
    const unsigned char *rpid;
    const double *rp_val;     // [rp_npat][9]
    const int *rp_mask;       // [rp_npat]
    int rp_npat;
    // hot-transfer kernels (HX): the usual patterns of P and R, their values in scalar registers.  phot[line parity] =
    // id of the even-column | id of the odd-column pattern << 8 (-1: none), with exactly the slots of the tensor-product
    // interpolation (0x1, 0x3 on even lines, 0x5, 0xF on odd ones), phv = their values in that order (as for
    // lmg_stencil_smooth_prolong); rhot = a pattern of R with all nine slots (-1: none), rhv = its values
    int phot[2];
    double phv[9];
    int rhot;
    double rhv[9];
    // CHEB: the (a_k, c_k) of sweep k + 1 of the Chebyshev step (last, so that every other field keeps its place)
    double cha[3], chc[3];
};

// HX (hot transfers, with PROL or REST): the correction x + P e is formed as each element arrives, from the usual pair
// of P in scalar registers where a whole wave line has it (else from the table in global memory) -- no 2 x 2 window per
// element stays live across the pattern staging and barrier; the restriction runs once per coarse node (a thread per
// node of the tile's inner part, 32 per wave line) instead of being carried by every fine element, with the frequent
// row of R in scalar registers where a whole wave has it.
// CHEB (Chebyshev polynomial smoother of degree S on D^-1 A): sweep k = 0 .. S - 1 is
//     d = a_k * d + c_k * (rdiag * (b - A x))   (k = 0: d = c_0 * (rdiag * (b - A x)), no add),   x = x + d
// with the coefficients in scalar registers and d of the elements a lane owns in its registers from sweep to sweep (a
// lane computes the same elements in every sweep, halo included, so d never travels).  The row sums, the transfers and
// the residual are those of the Jacobi pass; degree 1 is the Jacobi sweep with omega = c_0, bit for bit.
// Waves per SIMD a kernel is held to; 8 means at most 64 VGPRs.
//  - 16-wave workgroups, so that two of them share a CU -- the variants with the restriction had 65 - 67; the 64-line
//    turnaround, four lines per wave, needs 76 / 89 and spills under that bound.
//  - The 16-line restricting pass with hot transfers from a non-zero iterate: it had 57 registers while its prologue was a
//    chain of branches; with the straight-line prologue the scheduler, left to itself, spends 67 - 71 on its sweeps.
constexpr int tile_min_waves(int RR, int RBV, bool ZERO, bool PROL, bool REST, bool HX, bool CHEB)
{
    if (RR / RBV == 16 && (!PROL || HX) && !(PROL && REST && RBV == 4)) return 8;
    if (RR == 16 && REST && HX && !PROL && !ZERO && !CHEB) return 8;
    return 1;
}

// The forms that have a second body for tiles INSIDE the grid (INT, below): the Jacobi passes on two lines per wave -- the
// kernels a cycle launches on its mid-size levels.  -DLMG_TILE_GENERAL_ONLY: a probe build without it.
constexpr bool tile_has_interior(int S, int RR, int RBV, bool ZERO, bool PROL, bool REST, bool CHEB)
{
#ifdef LMG_TILE_GENERAL_ONLY
    return false;
#else
    // (not the 16-line restricting pass of one sweep from zero: with the second body 62 / 64 VGPRs become 65, 7 waves per SIMD)
    if (RR == 16 && REST && ZERO && S == 1) return false;
    return !CHEB && !(PROL && REST) && RBV == 2 && (RR == 16 || RR == 32);
#endif
}

// -DLMG_TILE_LDS_SIDES=1: a probe build whose window takes a line's left and right neighbours from LDS, not from DPP moves
#ifndef LMG_TILE_LDS_SIDES
#define LMG_TILE_LDS_SIDES 0
#endif

// The tile at (c0, y0) lies inside the grid: every element of its 64 x RR window is the row (line, column) it seems to
// be, and with a transfer every coarse index it forms lies inside the coarse vector with no clamp active.  Scalars only.
template <int H, int RR, bool PROL, bool REST>
__device__ __forceinline__ bool tile_is_interior(const TArgs &a, int c0, int y0)
{
    bool in = y0 >= 0 && y0 + RR <= a.lines && c0 >= 0 && c0 + kCols <= a.W && (int64_t)a.lines * a.W == a.n;
    if (PROL)     // the last window of the tile ends inside e_c: min(base, nc - 2) never bites
        in = in && a.W >= 2 * kCols &&
             (int64_t)((y0 + RR - 1) >> 1) * a.Wc + ((c0 + kCols - 1) >> 1) + a.Wc + 1 <= (int64_t)a.nc - 1;
    if (REST)     // the last coarse node of the inner part is a row of R
        in = in && (int64_t)(((y0 + RR - H - 1) & ~1) >> 1) * a.Wc + (((c0 + kCols - H - 1) & ~1) >> 1) < (int64_t)a.nc;
    return in;
}

template <int S, unsigned UM, bool RESID, bool ZERO, int RR, bool PROL = false, bool REST = false, int RBV = kRB, bool HX = false,
          bool CHEB = false>
__global__ void __launch_bounds__(RR / RBV * LMG_WAVE, tile_min_waves(RR, RBV, ZERO, PROL, REST, HX, CHEB))
stencil_tile_kernel(TArgs a)
{
    // PROL && REST: the turnaround of a repeated level visit -- the post-smoothing pass of visit k (correction, then
    // its sweeps) and the pre-smoothing pass of visit k + 1 (its sweeps, then the restriction) as one pass of S sweeps
    static_assert(!PROL || (!ZERO && (!RESID || REST)), "the correction is folded into post-smoothing passes only");
    static_assert(!REST || RESID, "the restriction replaces the store of the residual");
    // halo: one more with REST -- the residual has to be exact one line / column beyond the stored part
    constexpr int H = S + (RESID ? 1 : 0) - (ZERO ? 1 : 0) + (REST ? 1 : 0);
    constexpr int kWaves = RR / RBV, kBlock = kWaves * LMG_WAVE;
    static_assert(RR > 2 * H + 1 && kCols > 2 * H && RR % RBV == 0, "tile smaller than its halo / lines per wave");
    static_assert(!HX || PROL || REST, "hot transfers need a transfer");
    static_assert(!(REST && HX) || (RR - 2 * H + 1) / 2 <= RR / RBV * 2, "a thread per coarse node of the tile");
    // LDS holds the two iterate buffers only: right-hand side and pattern ids of a wave's own lines never change and
    // stay in its registers (32-line tiles: 39 KB instead of 60, i.e. four workgroups per CU instead of two).
    __shared__ double s_x[2][RR * kLS];
    __shared__ double s_val[kMaxPat * 9];
    __shared__ int s_mask[kMaxPat];
    __shared__ double s_rdiag[kMaxPat];
    __shared__ double s_pv[(PROL && !HX) ? kMaxPat * 4 : 1];
    __shared__ int s_pm[(PROL && !HX) ? kMaxPat : 1];
    __shared__ double s_rv[REST ? kMaxPat * 9 : 1];
    __shared__ int s_rm[REST ? kMaxPat : 1];

    const int t = threadIdx.x, lane = t & (LMG_WAVE - 1), wave = t >> 6;
    const int tx = (int)blockIdx.x % a.tiles_x, ty = (int)blockIdx.x / a.tiles_x;
    const int c0 = tx * (kCols - 2 * H) - H, y0 = ty * (RR - 2 * H) - H;
    const int n = a.n;
    const int64_t W = a.W;
    constexpr int RB = RBV;                                      // consecutive lines of the tile a wave owns
    constexpr bool DIAG = (UM & kMaskCorners) != 0;

    // One tile: stencil_tile_body.inc.  INT: the body of a tile for which tile_is_interior holds -- the same values from
    // the same instruction sequence per row, but every element is the row (line, column) it seems to be: its address is
    // the line's scalar base plus the lane, nothing is clamped, no validity selects, no row marks to test, and the
    // transfers' coarse indices need no clamp either.  Rows of any pattern, rows without a diagonal and waves that are
    // not all-hot take the same paths as in the general body.  One scalar branch per workgroup decides: 92 % of the
    // tiles of a 2049^2 level lie inside the grid, 83 % at 1025^2.
    if constexpr (tile_has_interior(S, RR, RBV, ZERO, PROL, REST, CHEB)) {
        if (tile_is_interior<H, RR, PROL, REST>(a, c0, y0)) {
            constexpr bool INT = true;
#include "stencil_tile_body.inc"
            return;
        }
    }
    constexpr bool INT = false;
#include "stencil_tile_body.inc"
}

int g_tile_rows = 16;       // lines per tile (16, 32; 0 = 32) on grids of fewer than g_tile_big_lines lines: more, smaller workgroups
                            // where a level is a handful of tiles (cfg#4 cycle 0.4725 -> 0.4687 ms, 1025^2 / 4 levels 0.1150 -> 0.1103,
                            // cfg#2 0.0728 -> 0.0706)
int g_tile_prol_wide_lines = 768;    // grids of at least this many lines: the pass with the correction on 8-wave workgroups
int g_tile_rows_big = 0;    // the same for grids of at least g_tile_big_lines lines
int g_tile_big_lines = 600;
int g_tile_hot_transfers = 1;       // the passes with a transfer folded in run the HX kernels
int g_tile_turnaround_rows = 0;     // lines per tile of the turnaround pass (32, 64; 0 = 64 on grids of at least
                                    // g_tile_big_lines lines, 32 below): its halo is s_post + s_pre + 2 lines
int g_tile_prol_wide_lines_hx = 1 << 30;    // g_tile_prol_wide_lines of the HX kernels: at 61 VGPRs the 16-wave variant
                                            // runs 8 waves / SIMD (4 lines per wave: 87 VGPRs, 5); cfg#4 cycle 0.4698 ->
                                            // 0.4539 ms without the 4-line variant at 2049^2

template <int S, unsigned UM, bool RESID, bool ZERO, int RR, bool PROL = false, bool REST = false, int RBV = kRB, bool HX = false,
          bool CHEB = false>
int launch5(TArgs a, hipStream_t st)
{
    constexpr int H = S + (RESID ? 1 : 0) - (ZERO ? 1 : 0) + (REST ? 1 : 0);
    a.tiles_x = (a.W + (kCols - 2 * H) - 1) / (kCols - 2 * H);
    a.tiles_y = (a.lines + (RR - 2 * H) - 1) / (RR - 2 * H);
    const int64_t grid = (int64_t)a.tiles_x * a.tiles_y;
    if (grid > 0x7fffffff) return LMG_ERR_CAPACITY;
    hipLaunchKernelGGL((stencil_tile_kernel<S, UM, RESID, ZERO, RR, PROL, REST, RBV, HX, CHEB>), dim3((unsigned)grid),
                       dim3(RR / RBV * LMG_WAVE), 0, st, a);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

static int tile_rows_for(const TArgs &a)
{
    const int rr = a.lines >= g_tile_big_lines ? g_tile_rows_big : g_tile_rows;
    return rr == 0 ? 32 : rr;     // measured in the cycle (cfg#4): 0.672 ms with 32-line tiles (16 waves), 0.688 with 16 (8 waves)
}

template <int S, unsigned UM, bool RESID, bool ZERO, bool PROL, bool REST, bool HX, bool CHEB = false>
int launch4x(TArgs a, hipStream_t st)
{
    if (tile_rows_for(a) == 16) return launch5<S, UM, RESID, ZERO, 16, PROL, REST, kRB, HX, CHEB>(a, st);
    // the pass with the correction needs 81 VGPRs: a 16-wave workgroup then fills a CU alone; on levels with many tiles
    // it runs 8 waves of four lines each (2049^2, 9-point: 69 instead of 81 us)
    if constexpr (PROL) {
        if (a.lines >= (HX ? g_tile_prol_wide_lines_hx : g_tile_prol_wide_lines))
            return launch5<S, UM, RESID, ZERO, 32, PROL, REST, 4, HX, CHEB>(a, st);
    }
    return launch5<S, UM, RESID, ZERO, 32, PROL, REST, kRB, HX, CHEB>(a, st);
}

template <int S, unsigned UM, bool RESID, bool ZERO, bool PROL = false, bool REST = false, bool CHEB = false>
int launch4(TArgs a, hipStream_t st)
{
    if constexpr (PROL || REST) {
        if (g_tile_hot_transfers) return launch4x<S, UM, RESID, ZERO, PROL, REST, true, CHEB>(a, st);
    }
    return launch4x<S, UM, RESID, ZERO, PROL, REST, false, CHEB>(a, st);
}

// The turnaround: x + P e, S = s_post + s_pre sweeps, b_coarse = R (b - A x) -- a halo of S + 2 lines and columns.  Its
// 64-line tiles are 16 waves of four lines (a wave cannot hold more than 1024 threads' worth of 2-line blocks).
template <int S, unsigned UM, bool HX>
int launch_turn3(TArgs a, hipStream_t st)
{
    const int rr = g_tile_turnaround_rows ? g_tile_turnaround_rows : (a.lines >= g_tile_big_lines ? 64 : 32);
    if (rr == 64) return launch5<S, UM, true, false, 64, true, true, 4, HX>(a, st);
    return launch5<S, UM, true, false, 32, true, true, kRB, HX>(a, st);
}

// (sweeps, residual, zero iterate, hot transfers) -> template arguments: exactly the combinations each entry point offers
template <unsigned UM, bool CHEB = false>
int launch_plain(TArgs a, int sweeps, bool resid, bool zero, hipStream_t st)
{
    return lmg_with_sweeps<1, 3>(sweeps, [&](auto s) {
        return lmg_with_flag(resid, [&](auto r) {
            return lmg_with_flag(zero, [&](auto z) {
                return launch4<LMG_CT(s), UM, LMG_CT(r), LMG_CT(z), false, false, CHEB>(a, st);
            });
        });
    });
}

template <unsigned UM, bool CHEB = false>
int launch_prol(TArgs a, int sweeps, hipStream_t st)
{
    return lmg_with_sweeps<1, 3>(sweeps, [&](auto s) { return launch4<LMG_CT(s), UM, false, false, true, false, CHEB>(a, st); });
}

template <unsigned UM, bool CHEB = false>
int launch_rest(TArgs a, int sweeps, bool zero, hipStream_t st)
{
    return lmg_with_sweeps<1, 3>(sweeps, [&](auto s) {
        return lmg_with_flag(zero, [&](auto z) { return launch4<LMG_CT(s), UM, true, LMG_CT(z), false, true, CHEB>(a, st); });
    });
}

template <unsigned UM>
int launch_turn(TArgs a, int sweeps, hipStream_t st)
{
    return lmg_with_sweeps<2, 6>(sweeps, [&](auto s) {
        return lmg_with_flag(g_tile_hot_transfers != 0, [&](auto hx) { return launch_turn3<LMG_CT(s), UM, LMG_CT(hx)>(a, st); });
    });
}

// The coefficient table of a Chebyshev step: h_coef = HOST pointer to (a_0, c_0, .., a_(degree-1), c_(degree-1)).  c_0
// stands in for omega in the shared argument rules.
bool cheby_coef_ok(int degree, const double *h_coef) { return degree >= 1 && degree <= 3 && h_coef != nullptr; }

// the fields only this pass has: the tiling that launch5 decides, and the table of a Chebyshev step (cheby_coef_ok)
TArgs own_fields(int degree, const double *h_coef)
{
    TArgs a;
    a.tiles_x = a.tiles_y = 0;
    for (int k = 0; k < 3; ++k) {
        a.cha[k] = h_coef && k < degree ? h_coef[2 * k] : 0.0;
        a.chc[k] = h_coef && k < degree ? h_coef[2 * k + 1] : 0.0;
    }
    return a;
}

// The plain, the correcting and the restricting pass, for both smoothers: h_coef == nullptr is weighted Jacobi, else a
// Chebyshev step of degree v.sweeps (the entry point has asked cheby_coef_ok).
int tiled_plain(const LmgOperator &op, const LmgSolve &v, const double *h_coef, void *stream)
{
    return lmg_fused_pass<kMask5, kMask9>(own_fields(v.sweeps, h_coef), op, v, nullptr, nullptr, [&](const TArgs &a, auto m) {
        return lmg_with_flag(h_coef != nullptr, [&](auto ch) {
            return launch_plain<LMG_CT(m), LMG_CT(ch)>(a, v.sweeps, v.r_out != nullptr, v.x_in == nullptr, lmg_stream(stream));
        });
    });
}

int tiled_prolong(const LmgOperator &op, const LmgSolve &v, const double *h_coef, const LmgProl &p, void *stream)
{
    return lmg_fused_pass<kMask5, kMask9>(own_fields(v.sweeps, h_coef), op, v, &p, nullptr, [&](const TArgs &a, auto m) {
        return lmg_with_flag(h_coef != nullptr, [&](auto ch) {
            return launch_prol<LMG_CT(m), LMG_CT(ch)>(a, v.sweeps, lmg_stream(stream));
        });
    });
}

int tiled_restrict(const LmgOperator &op, const LmgSolve &v, const double *h_coef, const LmgRest &r, void *stream)
{
    return lmg_fused_pass<kMask5, kMask9>(own_fields(v.sweeps, h_coef), op, v, nullptr, &r, [&](const TArgs &a, auto m) {
        return lmg_with_flag(h_coef != nullptr, [&](auto ch) {
            return launch_rest<LMG_CT(m), LMG_CT(ch)>(a, v.sweeps, v.x_in == nullptr, lmg_stream(stream));
        });
    });
}

}  // namespace

constexpr LmgTuneKey lmg_tune_tile[] = {
    lmg_tune_list("tile_rows", &g_tile_rows, 0, 16, 32),
    lmg_tune_list("tile_rows_big", &g_tile_rows_big, 0, 16, 32),
    lmg_tune_range("tile_big_lines", &g_tile_big_lines, 0),
    lmg_tune_range("tile_prol_wide_lines", &g_tile_prol_wide_lines, 0),
    lmg_tune_range("tile_prol_wide_lines_hx", &g_tile_prol_wide_lines_hx, 0),
    lmg_tune_list("tile_turnaround_rows", &g_tile_turnaround_rows, 0, 32, 64),
    lmg_tune_list("tile_hot_transfers", &g_tile_hot_transfers, 0, 1),
    kLmgTuneEnd,
};

extern "C" {

int lmg_stencil_smooth_tiled(int64_t n, int32_t line_stride, const uint8_t *pid, int32_t npat, const double *st_val,
                             const int32_t *st_mask, uint32_t union_mask, int32_t hot_pattern, const double *h_hot_val,
                             int sweeps, const double *x_in, const double *b, double omega, double *x_out, double *r_out,
                             void *stream)
{
    return tiled_plain({n, line_stride, pid, npat, st_val, st_mask, union_mask, hot_pattern, h_hot_val},
                       {sweeps, x_in, b, omega, x_out, r_out}, nullptr, stream);
}

int lmg_stencil_smooth_tiled_prolong(int64_t n, int32_t line_stride, const uint8_t *pid, int32_t npat, const double *st_val,
                                     const int32_t *st_mask, uint32_t union_mask, int32_t hot_pattern,
                                     const double *h_hot_val, int sweeps, const double *x_in, const double *b, double omega,
                                     double *x_out, int64_t n_coarse, int32_t coarse_stride, const double *e_coarse,
                                     const uint8_t *p_pid, int32_t p_npat, const double *p_val, const int32_t *p_mask,
                                     const int32_t *h_hot_pairs, const double *h_hot_pval, void *stream)
{
    return tiled_prolong({n, line_stride, pid, npat, st_val, st_mask, union_mask, hot_pattern, h_hot_val},
                         {sweeps, x_in, b, omega, x_out, nullptr}, nullptr,
                         {n_coarse, coarse_stride, e_coarse, p_pid, p_npat, p_val, p_mask, h_hot_pairs, h_hot_pval}, stream);
}

int lmg_stencil_smooth_tiled_restrict(int64_t n, int32_t line_stride, const uint8_t *pid, int32_t npat, const double *st_val,
                                      const int32_t *st_mask, uint32_t union_mask, int32_t hot_pattern,
                                      const double *h_hot_val, int sweeps, const double *x_in, const double *b, double omega,
                                      double *x_out, int64_t n_coarse, int32_t coarse_stride, double *b_coarse,
                                      const uint8_t *r_pid, int32_t r_npat, const double *r_val, const int32_t *r_mask,
                                      int32_t hot_r, const double *h_hot_rval, void *stream)
{
    return tiled_restrict({n, line_stride, pid, npat, st_val, st_mask, union_mask, hot_pattern, h_hot_val},
                          {sweeps, x_in, b, omega, x_out, nullptr}, nullptr,
                          {n_coarse, coarse_stride, b_coarse, r_pid, r_npat, r_val, r_mask, hot_r, h_hot_rval}, stream);
}

int lmg_stencil_smooth_tiled_turnaround(int64_t n, int32_t line_stride, const uint8_t *pid, int32_t npat, const double *st_val,
                                        const int32_t *st_mask, uint32_t union_mask, int32_t hot_pattern,
                                        const double *h_hot_val, int sweeps_post, int sweeps_pre, const double *x_in,
                                        const double *b, double omega, double *x_out, int64_t n_coarse, int32_t coarse_stride,
                                        const double *e_coarse, const uint8_t *p_pid, int32_t p_npat, const double *p_val,
                                        const int32_t *p_mask, const int32_t *h_hot_pairs, const double *h_hot_pval,
                                        double *b_coarse, const uint8_t *r_pid, int32_t r_npat, const double *r_val,
                                        const int32_t *r_mask, int32_t hot_r, const double *h_hot_rval, void *stream)
{
    // its own rule: two sweep counts, in front of the checks of the correcting and of the restricting pass
    if (sweeps_post < 1 || sweeps_post > 3 || sweeps_pre < 1 || sweeps_pre > 3) return LMG_ERR_ARG;
    const LmgProl p = {n_coarse, coarse_stride, e_coarse, p_pid, p_npat, p_val, p_mask, h_hot_pairs, h_hot_pval};
    const LmgRest r = {n_coarse, coarse_stride, b_coarse, r_pid, r_npat, r_val, r_mask, hot_r, h_hot_rval};
    return lmg_fused_pass<kMask5, kMask9>(own_fields(0, nullptr),
                                          {n, line_stride, pid, npat, st_val, st_mask, union_mask, hot_pattern, h_hot_val},
                                          {sweeps_post, x_in, b, omega, x_out, nullptr}, &p, &r, [&](const TArgs &a, auto m) {
                                              return launch_turn<LMG_CT(m)>(a, sweeps_post + sweeps_pre, lmg_stream(stream));
                                          });
}

int lmg_stencil_cheby_tiled(int64_t n, int32_t line_stride, const uint8_t *pid, int32_t npat, const double *st_val,
                            const int32_t *st_mask, uint32_t union_mask, int32_t hot_pattern, const double *h_hot_val,
                            int degree, const double *h_coef, const double *x_in, const double *b, double *x_out,
                            double *r_out, void *stream)
{
    if (!cheby_coef_ok(degree, h_coef)) return LMG_ERR_ARG;
    return tiled_plain({n, line_stride, pid, npat, st_val, st_mask, union_mask, hot_pattern, h_hot_val},
                       {degree, x_in, b, h_coef[1], x_out, r_out}, h_coef, stream);
}

int lmg_stencil_cheby_tiled_prolong(int64_t n, int32_t line_stride, const uint8_t *pid, int32_t npat, const double *st_val,
                                    const int32_t *st_mask, uint32_t union_mask, int32_t hot_pattern,
                                    const double *h_hot_val, int degree, const double *h_coef, const double *x_in,
                                    const double *b, double *x_out, int64_t n_coarse, int32_t coarse_stride,
                                    const double *e_coarse, const uint8_t *p_pid, int32_t p_npat, const double *p_val,
                                    const int32_t *p_mask, const int32_t *h_hot_pairs, const double *h_hot_pval, void *stream)
{
    if (!cheby_coef_ok(degree, h_coef)) return LMG_ERR_ARG;
    return tiled_prolong({n, line_stride, pid, npat, st_val, st_mask, union_mask, hot_pattern, h_hot_val},
                         {degree, x_in, b, h_coef[1], x_out, nullptr}, h_coef,
                         {n_coarse, coarse_stride, e_coarse, p_pid, p_npat, p_val, p_mask, h_hot_pairs, h_hot_pval}, stream);
}

int lmg_stencil_cheby_tiled_restrict(int64_t n, int32_t line_stride, const uint8_t *pid, int32_t npat, const double *st_val,
                                     const int32_t *st_mask, uint32_t union_mask, int32_t hot_pattern,
                                     const double *h_hot_val, int degree, const double *h_coef, const double *x_in,
                                     const double *b, double *x_out, int64_t n_coarse, int32_t coarse_stride,
                                     double *b_coarse, const uint8_t *r_pid, int32_t r_npat, const double *r_val,
                                     const int32_t *r_mask, int32_t hot_r, const double *h_hot_rval, void *stream)
{
    if (!cheby_coef_ok(degree, h_coef)) return LMG_ERR_ARG;
    return tiled_restrict({n, line_stride, pid, npat, st_val, st_mask, union_mask, hot_pattern, h_hot_val},
                          {degree, x_in, b, h_coef[1], x_out, nullptr}, h_coef,
                          {n_coarse, coarse_stride, b_coarse, r_pid, r_npat, r_val, r_mask, hot_r, h_hot_rval}, stream);
}

int lmg_stencil_smooth_tiled_supported(uint32_t union_mask)
{
    return union_mask == kMask5 || union_mask == kMask9;
}

}  // extern "C"
