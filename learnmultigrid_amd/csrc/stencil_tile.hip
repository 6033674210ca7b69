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
    const int rb0 = wave * RB;

    // ---- request: every global load of the prologue, from addresses that are valid whatever the element is ----------
    // (the rule and its reason: head of this file)
    struct Raw {                                                  // one element of a wave line as it comes out of memory
        double x, b;
        int pid, ppid, rpid;
        d2u e01, e23;                                             // PROL: the 2 x 2 coarse window, two 16-byte loads
    };
    Raw raw[RB];
    bool ok[RB];
    // PROL: bit 0 / 1: the first / second load of the window starts where the window does, bit 2 / 3: parity of the
    // element's own line / column -- one register per line instead of the 64-bit indices they come from
    int wf[PROL ? RB : 1];
    bool crow[(REST && !HX) ? RB : 1];                            // REST: the element carries a row of R
    // REST with HX: this thread's coarse node -- line t >> 5, column t & 31 of the even nodes of the inner part
    int rq = 0, rrow = H, rcol = H;
    bool rown = false, rhas = false;
    if (REST && HX) {
        const int ye0 = (y0 + H + 1) & ~1, xe0 = (c0 + H + 1) & ~1;   // (y0 + H, c0 + H >= 0)
        const int yf = ye0 + 2 * (t >> 5), xf = xe0 + 2 * (t & 31);
        rown = yf < y0 + RR - H && yf < a.lines && xf < c0 + kCols - H && xf < W;
        const int64_t jc = (int64_t)(yf >> 1) * a.Wc + (xf >> 1);
        rhas = rown && jc < a.nc;
        rq = (int)a.rpid[rhas ? jc : 0];
        rrow = rown ? yf - y0 : H;
        rcol = rown ? xf - c0 : H;
    }
    // PROL with HX: the usual pair of P as values in scalar registers (a select between two kernel arguments that the
    // compiler can still see as such becomes a load from the argument block, indexed by the lane: a round trip)
    int phot[2] = {-1, -1};
    double phv[9] = {};
    if (PROL && HX) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            phot[s] = a.phot[s];
            asm volatile("" : "+s"(phot[s]));
        }
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            phv[s] = a.phv[s];
            asm volatile("" : "+s"(phv[s]));
        }
    }
    auto request = [&](int k) {
        const int y = y0 + rb0 + k;
        const int64_t i = (int64_t)y * W + c0 + lane;
        // (linear validity: an element outside the lines 0 .. lines - 1 whose index is a row -- (-1, W) is row 0, (lines, -1)
        // row n - 1 -- is that row, which operators with an entry across a line end read)
        ok[k] = i >= 0 && i < n;
        const int64_t j = ok[k] ? i : 0;
        raw[k].x = ZERO ? 0.0 : a.x[j];
        raw[k].b = a.b[j];
        raw[k].pid = (int)a.pid[j];
        if (PROL) {
            // the element is row j of P whatever its place in the tile (a column outside [0, W) is an element of the
            // adjacent line): its own line and column decide the window.  On grids at least two tiles wide one step to
            // the neighbouring line is enough; narrower ones divide.
            const int c = c0 + lane;
            int yy, xx;
            if (a.W >= 2 * kCols) {                               // uniform
                yy = c < 0 ? y - 1 : (c >= a.W ? y + 1 : y);
                xx = c < 0 ? c + a.W : (c >= a.W ? c - a.W : c);
            } else {
                yy = (int)((unsigned)j / (unsigned)a.W);
                xx = (int)((unsigned)j - (unsigned)yy * (unsigned)a.W);
            }
            const int64_t base = (int64_t)(yy >> 1) * a.Wc + (xx >> 1);
            raw[k].ppid = (int)a.ppid[j];
            // slots 0, 1 and 2, 3 are neighbours in memory: two 16-byte loads (8-byte aligned is enough); slots a
            // pattern does not have may point anywhere inside the vector
            const int64_t b0 = ok[k] ? min(base, (int64_t)a.nc - 2) : 0, b1 = ok[k] ? min(base + a.Wc, (int64_t)a.nc - 2) : 0;
            raw[k].e01 = *reinterpret_cast<const d2u *>(a.ec + b0);
            raw[k].e23 = *reinterpret_cast<const d2u *>(a.ec + b1);
            wf[k] = (b0 == base ? 1 : 0) | (b1 == base + a.Wc ? 2 : 0) | ((yy & 1) << 2) | ((xx & 1) << 3);
        }
        if (REST && !HX) {
            // elements on (even line, even column) of the grid carry a row of R
            const int c = c0 + lane;
            crow[k] = ok[k] && !(y & 1) && !(c & 1) && c >= 0 && c < W;
            const int64_t jc = (int64_t)(y >> 1) * a.Wc + (c >> 1);
            raw[k].rpid = (int)a.rpid[(crow[k] && jc < a.nc) ? jc : 0];
        }
    };
    // The loaded values pass through empty asm statements: a load cannot sink into a branch behind one, and no use can
    // rise above it.  The last request comes first, so that the one wait stands in front of it.
    auto arrived = [&](int k) {
        if (PROL)
            asm volatile("" : "+v"(raw[k].ppid), "+v"(raw[k].e01.a), "+v"(raw[k].e01.b), "+v"(raw[k].e23.a), "+v"(raw[k].e23.b),
                              "+v"(wf[k]));
        if (REST && !HX) asm volatile("" : "+v"(raw[k].rpid));
        if (!ZERO) asm volatile("" : "+v"(raw[k].x));
        asm volatile("" : "+v"(raw[k].b), "+v"(raw[k].pid));
    };
    // four lines with their windows in flight are 56 registers: those kernels ask for their lines one at a time
    constexpr int RG = (PROL && (RB > 2 || REST)) ? 1 : RB;
    static_assert(RB % RG == 0, "whole groups of lines");
#pragma unroll
    for (int k = 0; k < RG; ++k) request(k);
    // this thread's element of every table the workgroup stages (a block is at least as long as any table but the two
    // with nine values per pattern: their tail, if there is one, follows the consume step)
    static_assert(kBlock >= kMaxPat * 4, "one element of the short tables per thread");
    const int tv_n = a.npat * 9, tr_n = REST ? a.rp_npat * 9 : 1, tp_n = (PROL && !HX) ? a.pp_npat * 4 : 1;
    const int tm_i = min(t, a.npat - 1);
    double raw_sv = a.st_val[min(t, tv_n - 1)];                   // (staged in place: see lmg_common.hpp)
    int raw_sm = a.st_mask[tm_i];
    double raw_sd = a.st_val[tm_i * 9 + 4];                       // the diagonal: inside the table whatever the mask says
    double raw_rv = 0.0, raw_pv = 0.0;
    int raw_rm = 0, raw_pm = 0;
    if (REST) {
        raw_rv = a.rp_val[min(t, tr_n - 1)];
        raw_rm = a.rp_mask[min(t, a.rp_npat - 1)];
    }
    if (PROL && !HX) {
        raw_pv = a.pp_val[min(t, tp_n - 1)];
        raw_pm = a.pp_mask[min(t, a.pp_npat - 1)];
    }
    // (what needs no load goes here, behind the requests)
    for (int i = t; i < 2 * RR; i += kBlock) {                    // guard columns of both iterate buffers
        const int r = i >> 1, g = (i & 1) ? kLS - 1 : 0;
        s_x[0][r * kLS + g] = 0.0;
        s_x[1][r * kLS + g] = 0.0;
    }

    // ---- consume: nothing above this line uses a loaded value --------------------------------------------------------
    if (PROL && !HX) asm volatile("" : "+v"(raw_pv), "+v"(raw_pm));
    if (REST) asm volatile("" : "+v"(raw_rv), "+v"(raw_rm));
    asm volatile("" : "+v"(raw_sv), "+v"(raw_sm), "+v"(raw_sd));
#pragma unroll
    for (int k = RG - 1; k >= 0; --k) arrived(k);
    if (REST && HX) asm volatile("" : "+v"(rq));
    // (the tables' copies first: their registers are free before the lines need theirs; the reciprocals last, when the
    // lines' are free)
    if (t < tv_n) s_val[t] = raw_sv;
    if (REST) {
        if (t < tr_n) s_rv[t] = raw_rv;
        if (t < a.rp_npat) s_rm[t] = raw_rm;
    }
    if (PROL && !HX) {
        if (t < tp_n) s_pv[t] = raw_pv;
        if (t < a.pp_npat) s_pm[t] = raw_pm;
    }
    double lx[RB], bk[RB];
    int pk[RB];                                                   // pattern id | 0x100 where the element is a row of the matrix
    double le[(PROL && !HX) ? RB : 1][4];                         // PROL: the 2 x 2 coarse window of every element
    int lq[PROL ? RB : 1];                                        //       and its pattern id in P
    int lr[(REST && !HX) ? RB : 1];                               // REST: the id of R's row | 0x100 where the element has one
    if (REST && HX) rq = rhas ? (rq & 0xff) : 0;
    auto consume = [&](int k) {
        lx[k] = (!ZERO && ok[k]) ? raw[k].x : 0.0;
        bk[k] = ok[k] ? raw[k].b : 0.0;
        pk[k] = ok[k] ? ((raw[k].pid & 0xff) | 0x100) : 0;  // (& 0xff: behind the asm statement a byte is any int)
        if (PROL) {
            lq[k] = ok[k] ? (raw[k].ppid & 0xff) : 0;
            const d2u e01 = raw[k].e01, e23 = raw[k].e23;
            // (a window clamped at the end of the vector starts one element early: its first slot is the second value)
            const double w0 = (wf[k] & 1) ? e01.a : e01.b, w1 = e01.b, w2 = (wf[k] & 2) ? e23.a : e23.b, w3 = e23.b;
            if (!HX) {
                le[k][0] = w0;
                le[k][1] = w1;
                le[k][2] = w2;
                le[k][3] = w3;
            } else {
                // x + P e now: the sums of lmg_rpat_sweep_grid(SPMV, alpha = 1, beta = 1) in the same order
                const int yl = (wf[k] >> 2) & 1, xl = (wf[k] >> 3) & 1;
                // (read first, selected after: a select between two reads turns into one indexed read)
                const int h0 = phot[0], h1 = phot[1];
                const double p0 = phv[0], p1 = phv[1], p2 = phv[2], p3 = phv[3], p4 = phv[4], p5 = phv[5], p6 = phv[6], p7 = phv[7],
                             p8 = phv[8];
                const int hp = yl ? h1 : h0;
                const bool hotk = !ok[k] || (hp >= 0 && lq[k] == ((xl ? hp >> 8 : hp) & 0xff));
                double acc = 0.0;
                if (__all(hotk)) {                                // wave-uniform: the usual pair, slots 0 (1) (2) (3)
                    const double v0 = yl ? (xl ? p5 : p3) : (xl ? p1 : p0);
                    const double v1 = yl ? p6 : p2, v2 = xl ? p7 : p4;
                    acc = acc + v0 * w0;
                    double tv = acc + v1 * w1;
                    acc = xl ? tv : acc;
                    tv = acc + v2 * w2;
                    acc = yl ? tv : acc;
                    tv = acc + p8 * w3;
                    acc = (xl & yl) ? tv : acc;
                } else {
                    // (the one round trip left behind the wait: P's own row, which waves of the usual pair never ask for)
                    const int q = lq[k], m = a.pp_mask[q];
                    const double w[4] = {w0, w1, w2, w3};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const double tv = acc + a.pp_val[q * 4 + s] * w[s];
                        acc = ((m >> s) & 1) ? tv : acc;
                    }
                }
                lx[k] = (pk[k] >> 8) ? lx[k] + acc : 0.0;
            }
        }
        if (REST && !HX) lr[k] = crow[k] ? ((raw[k].rpid & 0xff) | 0x100) : 0;
    };
#pragma unroll
    for (int k = 0; k < RG; ++k) consume(k);
#pragma unroll
    for (int g = RG; g < RB; g += RG) {                           // (the remaining groups: a round trip each)
#pragma unroll
        for (int k = g; k < g + RG; ++k) request(k);
#pragma unroll
        for (int k = g + RG - 1; k >= g; --k) arrived(k);
#pragma unroll
        for (int k = g; k < g + RG; ++k) consume(k);
    }
    if (t < a.npat) {
        const int m = raw_sm;
        const double dg = (m & 16) ? raw_sd : 0.0;
        s_rdiag[t] = dg != 0.0 ? 1.0 / dg : 0.0;
        s_mask[t] = dg == 0.0 ? (m | (1 << 16)) : m;             // bit 16: no usable diagonal -> copy x
    }
    if constexpr (kBlock < kMaxPat * 9) {                         // more than kBlock / 9 patterns: the tails
        for (int i = t + kBlock; i < tv_n; i += kBlock) s_val[i] = a.st_val[i];
        if (REST)
            for (int i = t + kBlock; i < tr_n; i += kBlock) s_rv[i] = a.rp_val[i];
    }
    if (PROL && !HX) {
        __syncthreads();
        // x + P e: the sums of lmg_rpat_sweep_grid(SPMV, alpha = 1, beta = 1) in the same order
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const int m = s_pm[lq[k]];
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double tv = acc + s_pv[lq[k] * 4 + q] * le[k][q];
                acc = ((m >> q) & 1) ? tv : acc;
            }
            lx[k] = (pk[k] >> 8) ? lx[k] + acc : 0.0;
        }
    }
    const int hot = a.hot >= 0 ? (a.hot | 0x100) : -1;
    bool mine = true;
#pragma unroll
    for (int k = 0; k < RB; ++k) {
        s_x[0][(rb0 + k) * kLS + 1 + lane] = lx[k];
        s_x[1][(rb0 + k) * kLS + 1 + lane] = 0.0;
        mine = mine && (pk[k] == hot || !(pk[k] >> 8));          // (elements outside the matrix are not stored)
    }
    // every lane of every line of this wave holds the frequent pattern: its values sit in scalar registers
    const bool all_hot = __all(mine);
    __syncthreads();

    const double omega = a.omega;
    double dk[CHEB ? RB : 1];                                     // CHEB: d of the lane's elements
    double hv[9];
#pragma unroll
    for (int s = 0; s < 9; ++s) hv[s] = a.hot_val[s];
    const double hrd = a.hot_rdiag;

    // A wave slides a three-line window down its lines: the centre values of a line come from LDS (one 8-byte read
    // per lane), its left / right neighbours from the neighbouring lanes (DPP; lanes 0 / 63 get the zero of the
    // guard columns -- they are halo), so a line costs one LDS read instead of nine.
    struct Win { double m, c, p; };
    auto line = [&](const double *src, int r, bool sides) -> Win {
        Win w;
        w.c = src[r * kLS + 1 + lane];
        w.m = sides ? dpp_lower<true>(w.c) : 0.0;
        w.p = sides ? dpp_upper<true>(w.c) : 0.0;
        return w;
    };
    // A x of the centre line of (u, c, d) for this lane, slot order = column order
    auto apply = [&](const Win &u, const Win &c, const Win &d, int p, bool hotp) -> double {
        const double w[9] = {u.m, u.c, u.p, c.m, c.c, c.p, d.m, d.c, d.p};
        double acc = 0.0;
        if (hotp) {
#pragma unroll
            for (int s = 0; s < 9; ++s)
                if ((UM >> s) & 1u) acc = acc + hv[s] * w[s];
        } else {
            const int q = p & 0xff, m = s_mask[q];
#pragma unroll
            for (int s = 0; s < 9; ++s) {
                if (!((UM >> s) & 1u)) continue;
                const double tv = acc + s_val[q * 9 + s] * w[s];
                acc = ((m >> s) & 1) ? tv : acc;
            }
        }
        return acc;
    };
    // The wave's block of RB lines, straight-line: all its lines are read first, then either the frequent pattern
    // everywhere or every line through the pattern table -- no branch inside either path, so the LDS latencies and
    // the dependent sums of the RB lines overlap.  Lines outside [lo, hi) are computed from clamped (meaningless)
    // neighbours and not kept.
    auto block = [&](const double *src, int lo, int hi, auto &&emit) {
        Win ln[RB + 2];
#pragma unroll
        for (int j = 0; j < RB + 2; ++j) {
            const int rr = min(max(rb0 - 1 + j, 0), RR - 1);
            ln[j] = line(src, rr, DIAG || (j >= 1 && j <= RB));
        }
        if (all_hot) {                                             // wave-uniform
#pragma unroll
            for (int k = 0; k < RB; ++k) {
                const double acc = apply(ln[k], ln[k + 1], ln[k + 2], pk[k], true);
                emit(k, rb0 + k >= lo && rb0 + k < hi, true, ln[k + 1].c, acc);
            }
        } else {
#pragma unroll
            for (int k = 0; k < RB; ++k) {
                const double acc = apply(ln[k], ln[k + 1], ln[k + 2], pk[k], false);
                emit(k, rb0 + k >= lo && rb0 + k < hi, false, ln[k + 1].c, acc);
            }
        }
    };

    // ---- the sweeps: iterate s goes from buffer (s - 1) & 1 to buffer s & 1 -------------------------------------
#pragma unroll
    for (int s = 1; s <= S; ++s) {
        const double *src = s_x[(s - 1) & 1];
        double *dst = s_x[s & 1];
        if (CHEB && ZERO && s == 1) {
            // first sweep from a zero iterate: x = d = c_0 * (D^-1 b)
#pragma unroll
            for (int k = 0; k < RB; ++k) {
                dk[k] = a.chc[0] * (s_rdiag[pk[k] & 0xff] * bk[k]);
                dst[(rb0 + k) * kLS + 1 + lane] = (pk[k] >> 8) ? dk[k] : 0.0;
            }
        } else if (CHEB) {
            const double ca = a.cha[s - 1], cc = a.chc[s - 1];
            const bool first = s == 1;
            block(src, 1, RR - 1, [&](int k, bool keep, bool hotp, double xc, double acc) {
                const double res = bk[k] - acc;
                const int q = pk[k] & 0xff;
                const bool nodiag = !hotp && (s_mask[q] >> 16);
                const double z = (hotp ? hrd : s_rdiag[q]) * res;
                const double dn = first ? cc * z : ca * dk[k] + cc * z;
                dk[k] = nodiag ? 0.0 : dn;
                const double nx = nodiag ? xc : xc + dn;
                if (keep) dst[(rb0 + k) * kLS + 1 + lane] = (pk[k] >> 8) ? nx : 0.0;
            });
        } else if (ZERO && s == 1) {
            // first sweep from a zero iterate: x = omega * (D^-1 b) on every line (lmg_vmul's bits)
#pragma unroll
            for (int k = 0; k < RB; ++k)
                dst[(rb0 + k) * kLS + 1 + lane] = (pk[k] >> 8) ? omega * (s_rdiag[pk[k] & 0xff] * bk[k]) : 0.0;
        } else {
            // (lines 0 and RR - 1 have no line above / below)
            block(src, 1, RR - 1, [&](int k, bool keep, bool hotp, double xc, double acc) {
                const double res = bk[k] - acc;
                double nx;
                if (hotp) {
                    nx = xc + omega * (hrd * res);
                } else {
                    const int q = pk[k] & 0xff;
                    nx = (s_mask[q] >> 16) ? xc : xc + omega * (s_rdiag[q] * res);
                }
                if (keep) dst[(rb0 + k) * kLS + 1 + lane] = (pk[k] >> 8) ? nx : 0.0;
            });
        }
        __syncthreads();
    }

    // ---- outputs: the inner part of the tile, inside the line, rows of the matrix --------------------------------
    const double *fin = s_x[S & 1];
    const bool col_ok = lane >= H && lane < kCols - H && c0 + lane >= 0 && c0 + lane < W;
    if (REST) {
        // the residual goes to the other LDS buffer (all lines but the first and the last: exact where it is read),
        // then every element that carries a row of R sums its nine entries in column order -- the sums of
        // lmg_rpat_sweep_grid(SPMV, alpha = 1, beta = 0)
        double *rl = s_x[(S + 1) & 1];
        block(fin, 1, RR - 1, [&](int k, bool keep, bool, double xc, double acc) {
            const int r = rb0 + k;
            if (keep) rl[r * kLS + 1 + lane] = bk[k] - acc;
            if (r >= H && r < RR - H && col_ok && (pk[k] >> 8)) a.out[(int64_t)(y0 + r) * W + c0 + lane] = xc;
        });
        __syncthreads();
        if (HX) {
            // a thread per coarse node; waves without one have nothing left to do
            if (__any(rown)) {
                const double *p = rl + rrow * kLS + 1 + rcol;
                double acc = 0.0;
                if (__all(!rown || rq == a.rhot)) {
#pragma unroll
                    for (int e = 0; e < 9; ++e) acc = acc + a.rhv[e] * p[(e / 3 - 1) * kLS + e % 3 - 1];
                } else {
                    const int m = s_rm[rq];
#pragma unroll
                    for (int e = 0; e < 9; ++e) {
                        const double tv = acc + s_rv[rq * 9 + e] * p[(e / 3 - 1) * kLS + e % 3 - 1];
                        acc = ((m >> e) & 1) ? tv : acc;
                    }
                }
                if (rown) a.bc[(int64_t)((y0 + rrow) >> 1) * a.Wc + ((c0 + rcol) >> 1)] = acc;
            }
            return;
        }
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const int r = rb0 + k;
            const int q = lr[k] & 0xff, m = s_rm[q];
            double acc = 0.0;
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                const int rr = min(max(r + e / 3 - 1, 0), RR - 1);
                const double tv = acc + s_rv[q * 9 + e] * rl[rr * kLS + 1 + lane + e % 3 - 1];
                acc = ((m >> e) & 1) ? tv : acc;
            }
            if ((lr[k] >> 8) && r >= H && r < RR - H && col_ok)
                a.bc[(int64_t)((y0 + r) >> 1) * a.Wc + ((c0 + lane) >> 1)] = acc;
        }
    } else if (RESID) {
        block(fin, H, RR - H, [&](int k, bool keep, bool, double xc, double acc) {
            const int64_t i = (int64_t)(y0 + rb0 + k) * W + c0 + lane;
            if (keep && col_ok && (pk[k] >> 8)) {
                a.out[i] = xc;
                a.r[i] = bk[k] - acc;
            }
        });
    } else {
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const int r = rb0 + k;
            if (r >= H && r < RR - H && col_ok && (pk[k] >> 8))
                a.out[(int64_t)(y0 + r) * W + c0 + lane] = fin[r * kLS + 1 + lane];
        }
    }
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
