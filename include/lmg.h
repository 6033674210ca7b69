/*
 * lmg.h -- C ABI of the MI355X (gfx950) multigrid V-cycle kernels.
 *
 * This is the drop-in boundary for the hot path of claudiotomasi/LearnMultigrid
 * (learn_multigrid/solvers/Multigrid.py:36-124).  The reference is pure Python
 * and has no FFI of its own; each entry point below replaces one SciPy / pyamg
 * call made on that path and cites it (paths relative to /root/reference).
 * INTEGRATION.md shows the ctypes binding a maintainer adds on the Python side.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++ / torch types.
 *   - Every `const T*` / `T*` named d_* or documented "device" is a DEVICE pointer
 *     owned by the caller; the library never allocates, frees or synchronises
 *     inside a launch function (graph-capture safe) -- scratch is passed in.
 *   - CSR: int32 rowptr[n+1], int32 colidx[nnz], fp64 vals[nnz]; array bases must
 *     be 16-byte aligned (LMG_ERR_ALIGN otherwise).  Rows are accumulated in
 *     storage order with separate multiply and add roundings (no FMA contraction),
 *     which makes SpMV / Jacobi / Gauss-Seidel bit-identical to SciPy's
 *     csr_matvec and to pyamg's sweep on sorted CSR.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - Return value: LMG_OK (0) or a negative lmg_status; no exceptions cross the ABI.
 */
#ifndef LMG_H
#define LMG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMG_VERSION 100 /* 0.1.0 */

typedef enum {
    LMG_OK = 0,
    LMG_ERR_ARG = -1,       /* null pointer / negative size / bad enum            */
    LMG_ERR_ALIGN = -2,     /* array base not 16-byte aligned                     */
    LMG_ERR_LAUNCH = -3,    /* HIP reported a launch / runtime error              */
    LMG_ERR_CAPACITY = -4,  /* a row exceeds what the kernel's LDS tile can hold  */
    LMG_ERR_NODEVICE = -5   /* no HIP device visible                              */
} lmg_status;

int lmg_version(void);
const char *lmg_status_string(int status);
/* Number of visible HIP devices, or a negative lmg_status. */
int lmg_device_count(void);

/* Runtime tuning knobs: kernel variant selection and launch geometry, for A/B runs (bench.py, tools/) and for the
 * parity tests, which force the instantiations a launcher would only pick on very large operators.  Both calls
 * answer LMG_ERR_ARG to a key that is not listed here, lmg_tune_set also to a value it does not accept (and then
 * changes nothing); lmg_tune_get returns the value.  [default]
 *   key                        accepts        meaning
 *   "sweep_variant"            0..6      [0]  tile geometry of the plain-CSR sweeps; 0 = from the average row length
 *   "pcsr_ju"                  0 1 3 5 101 102  [0]  row entries per step of the packed sweeps; 0 = from the average
 *                                             row length.  101, 102 = TIMING PROBES, not sweeps: the kernel of 1 with
 *                                             the gathers of x left out (101: the column index stands in for x[column])
 *                                             and with the staging of the tile left out as well (102: whatever LDS
 *                                             holds).  The output vectors are written but are NOT the sweep's result.
 *                                             Only for the uint16-column / uint8-value encoding on 512-row tiles;
 *                                             lmg_pcsr_sweep answers LMG_ERR_ARG for every other twin while one is set.
 *   "rpat_variant"             0..4      [0]  geometry of the row-pattern sweeps; 0 = from the longest pattern
 *                                             (a value >= 1000 sets "rpat_nt_rows" instead: bench.py's spelling)
 *   "rpat_nt_rows"             >= 1      [8388608]  rows from which the row-pattern sweeps' streams bypass the caches
 *   "stencil_nt_rows"          >= 1      [8388608]  the same for the stencil sweeps
 *   "stencil_wgs_per_cu"       0..8      [0]  workgroups per CU of the stencil sweeps; 0 = occupancy query
 *   "fused_seg_lines"          >= 0      [0]  lines per segment of the register-fused passes; 0 = chosen per launch
 *   "fused_seg_min_lines"      >= 0      [0]  ... applied to grids of at least this many lines
 *   "fused_seg_max_lines"      >= 0      [2147483647]  ... and at most this many
 *   "fused_seg_lines_prol"     >= 0      [0]  lines per segment of the pass with the correction folded in; 0 = as the others
 *   "fused_seg_lines_rest"     >= 0      [0]  ... with the restriction folded in
 *   "fused_pf"                 0 2       [0]  kept for old scripts: stored, read by nothing
 *   "fused_want_waves"         >= 1      [5120]  waves a register-fused launch aims at when it cuts segments
 *   "fused_want_waves_rest3"   >= 1      [2700]  ... for three sweeps with a transfer folded in
 *   "fused_floor_halos"        >= 1      [4]  shortest segment, in halos
 *   "fused_balance"            0 1       [1]  shorter segments for the items that run the slower bodies
 *   "fused_slow_pct"           10..100   [55] their steps, per cent of a normal item's
 *   "fused_fast"               0 1       [1]  0: every wave runs the general body
 *   "tile_rows"                0 16 32   [16] lines per tile of the tiled passes on grids below "tile_big_lines"; 0 = 32
 *   "tile_rows_big"            0 16 32   [0]  ... on grids from "tile_big_lines" lines
 *   "tile_big_lines"           >= 0      [600]
 *   "tile_prol_wide_lines"     >= 0      [768]  lines from which the correcting tiled pass runs 8 waves of four lines
 *   "tile_prol_wide_lines_hx"  >= 0      [1073741824]  the same for its hot-transfer kernels
 *   "tile_turnaround_rows"     0 32 64   [0]  lines per tile of the turnaround pass; 0 = 64 from "tile_big_lines" lines, else 32
 *   "tile_hot_transfers"       0 1       [1]  passes with a transfer folded in run the hot-transfer kernels
 *   "dia_rows"                 0 32 64   [0]  lines per tile of lmg_dia_smooth; 0 = 32
 *   "sell_nt"                  -1..1     [-1] nontemporal streams of the sliced-ELL sweeps: -1 by size, 0 never, 1 always
 *   "sell_ju"                  0 5 7 8 10  [0]  row entries in flight there; 0 = from the longest row
 *   "gsw_max_sweeps"           1..4      [4]  Gauss-Seidel sweeps pipelined in one launch
 *   "gsw_multi_max_rows"       >= 0      [8000000]  ... on levels of at most this many rows (register bands)
 *   "gsw_lds"                  -1..1     [-1] bands staged through LDS: -1 / 1 wherever possible, 0 never
 *   "gsw_lds9"                 0 1       [1]  ... for 9-point operators too
 *   "gsw_lds_multi"            0 1       [1]  ... with the sweeps of a step pipelined in one launch
 *   "gs_single_max"            >= 1      [2048]  widest row set the one-workgroup Gauss-Seidel executor takes */
int lmg_tune_set(const char *key, int value);
int lmg_tune_get(const char *key);

/* ---- fine-level sweeps ---------------------------------------------------------
 * Number of fp64 partial sums lmg_csr_residual_norm2 / lmg_dot need as scratch. */
int64_t lmg_partials_count(int64_t n);

/* r = b - A x  and  *d_norm2 = sum_i r_i^2 (deterministic two-stage reduction).
 * Replaces `rhs - A.dot(u)` + `np.linalg.norm` (Multigrid.py:62-63,:90; Jacobi.py:28-29).
 * d_r may be NULL (norm only); d_partials/d_norm2 may both be NULL (residual only). */
int lmg_csr_residual_norm2(int64_t n, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                           const double *d_vals, const double *d_x, const double *d_b, double *d_r,
                           double *d_partials, double *d_norm2, void *stream);

/* x_out = x_in + omega * ((1/a_ii) * (b - A x_in)); rows without a diagonal copy x_in.
 * omega = 1 is the reference update `solution += inv_d * residual_vector`
 * (Jacobi.py:22-35).  x_out must not alias x_in. */
int lmg_csr_jacobi(int64_t n, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                   const double *d_vals, const double *d_x_in, const double *d_b, double omega,
                   double *d_x_out, void *stream);

/* y = alpha * (A x) + beta * y  (beta == 0 never reads y).
 * Restriction  r_c = P^T r  (Multigrid.py:93) with A := R = P^T stored as CSR;
 * prolongation u += P e     (Multigrid.py:115) with alpha = beta = 1. */
int lmg_csr_spmv(int64_t n_rows, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                 const double *d_vals, const double *d_x, double *d_y, double alpha, double beta,
                 void *stream);

/* ---- packed CSR ("PCSR") sweeps ---------------------------------------------------
 * Lossless re-encoding of a CSR matrix, built once at setup (learnmultigrid_amd/ops.py
 * PackedCSR shows how), that keeps the entry order -- results are bit-identical to the CSR
 * entry points above -- and moves fewer bytes:
 *   d_rowlen[n]          uint8 row lengths (rows longer than 255 entries: not packable)
 *   d_tile_base[T+1]     int32 entry offset of every tile of `tile_rows` rows (512 by default
 *                        = lmg_pcsr_tile_rows(); 128 or 64 for matrices with long rows)
 *   d_col                colmode 0: uint16 (column - d_tile_colbase[tile]); 1: int32 column
 *   d_val                valmode 0: uint8 index into d_dict (ndict <= 256); 1: uint16 index
 *                        (ndict <= 65536); 2: raw fp64 (d_dict unused)
 * d_col / d_val are 16-byte aligned and padded with >= 16 readable bytes; tile_cap is the
 * largest number of entries in one tile.  mode: 0 residual (+norm), 1 Jacobi, 2 SpMV, with
 * the argument meaning of lmg_csr_residual_norm2 / lmg_csr_jacobi (alpha = omega) /
 * lmg_csr_spmv.  LMG_ERR_CAPACITY if a tile does not fit the LDS budget (use the CSR path). */
int lmg_pcsr_tile_rows(void);
int lmg_pcsr_sweep(int mode, int64_t n, int64_t nnz, int32_t tile_rows, int32_t tile_cap,
                   const int32_t *d_tile_base,
                   const int32_t *d_tile_colbase, const uint8_t *d_rowlen, const void *d_col,
                   int colmode, const void *d_val, int valmode, const double *d_dict, int32_t ndict,
                   const double *d_x, const double *d_b, double *d_out, double alpha, double beta,
                   double *d_partials, double *d_norm2, void *stream);

/* ---- row-pattern ("RPAT") sweeps ---------------------------------------------------
 * Second lossless twin, for matrices whose rows repeat when written as (length; column - row
 * index and value bits of every entry, in storage order): assembled grid operators.  Each
 * distinct row is stored once, every row carries a uint8 pattern id:
 *   d_pid[n]                 pattern of every row
 *   d_pat_ptr[npat+1], d_pat_off[nent], d_pat_val[nent]   the patterns (CSR-like; off = col - row)
 * Limits from lmg_rpat_limits (255 patterns, 1024 entries in total; held in LDS).  Same modes,
 * argument meaning and bits as lmg_pcsr_sweep; max_len = longest pattern (picks the unrolling).
 * d_partials needs lmg_partials_count(n) doubles.
 * Building (learnmultigrid_amd/ops.py RowPatterns.from_csr is the calling sequence):
 *   lmg_rpat_row_hash   64-bit hash of every row's pattern
 *   -- distinct hashes with lmg_value_set_insert, ids with lmg_value_encode --
 *   lmg_rpat_claim      d_rep[p] (pre-set to -1) = some row with pattern id p
 *   lmg_rpat_verify     compares EVERY row with its pattern entry by entry (and its columns with
 *                       [0, ncols)); *d_mismatch != 0 means the format must not be used. */
int lmg_rpat_limits(int32_t *max_patterns, int32_t *max_entries);
int lmg_rpat_sweep(int mode, int64_t n, const uint8_t *d_pid, int32_t npat, int32_t nent, int32_t max_len,
                   const int32_t *d_pat_ptr, const int32_t *d_pat_off, const double *d_pat_val,
                   const double *d_x, const double *d_b, double *d_out, double alpha, double beta,
                   double *d_partials, double *d_norm2, void *stream);
int lmg_rpat_row_hash(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                      uint64_t *d_hash, void *stream);
int lmg_rpat_claim(int64_t n, const uint8_t *d_pid, int32_t *d_rep, void *stream);
int lmg_rpat_verify(int64_t n, int64_t ncols, const int32_t *d_rowptr, const int32_t *d_colidx,
                    const double *d_vals, const uint8_t *d_pid, int32_t npat, const int32_t *d_pat_ptr,
                    const int32_t *d_pat_off, const double *d_pat_val, int32_t *d_mismatch, void *stream);

/* Row patterns of RECTANGULAR grid operators (transfers between nested grids), SpMV only.  A pattern
 * then stores  column - base(row)  with, for y = row / row_len and x = row % row_len,
 *     base(row) = (y >> ysh) * col_stride + ((x >> xsh) << xshl),
 * h_grid_map = HOST pointer to {row_len, col_stride, ysh, xsh, xshl} (NULL or row_len 0: base(row) =
 * row, i.e. the functions above).  Restriction R = P^T of a tensor-product interpolator between a
 * Wf x Wf and a Wc x Wc grid: {Wc, 2 Wf, 0, 0, 1}; its prolongation P: {Wf, Wc, 1, 1, 0}; 1-D
 * transfers: row_len > number of rows.  The format stays a verified lossless re-encoding: the builder
 * (ops.RowPatterns.from_csr(A, grid_map)) tries a map, and lmg_rpat_verify_grid checks every entry.
 * u += P e and r_c = R r then move the vectors and one byte per row instead of 10-12 bytes per entry.
 * Replaces the same SciPy calls as lmg_csr_spmv (Multigrid.py:93, :115). */
int lmg_rpat_sweep_grid(int mode, int64_t n, const int32_t *h_grid_map, const uint8_t *d_pid, int32_t npat,
                        int32_t nent, int32_t max_len, const int32_t *d_pat_ptr, const int32_t *d_pat_off,
                        const double *d_pat_val, const double *d_x, const double *d_b, double *d_out,
                        double alpha, double beta, double *d_partials, double *d_norm2, void *stream);
int lmg_rpat_row_hash_grid(int64_t n, const int32_t *h_grid_map, const int32_t *d_rowptr,
                           const int32_t *d_colidx, const double *d_vals, uint64_t *d_hash, void *stream);
int lmg_rpat_verify_grid(int64_t n, int64_t ncols, const int32_t *h_grid_map, const int32_t *d_rowptr,
                         const int32_t *d_colidx, const double *d_vals, const uint8_t *d_pid, int32_t npat,
                         const int32_t *d_pat_ptr, const int32_t *d_pat_off, const double *d_pat_val,
                         int32_t *d_mismatch, void *stream);

/* ---- grid-stencil sweeps: row-pattern matrices whose patterns are 3x3 stencils ------------
 * A row-pattern matrix (d_pid as above) qualifies when every entry of every pattern sits at
 * column - row = c * line_stride + d with c, d in {-1, 0, 1} and every pattern lists its entries in
 * ascending column order: the 5-point operator of configs #2 / #4, its 9-point Galerkin
 * coarsenings, tridiagonal 1-D operators.  The pattern table is then stored by SLOT:
 *   d_st_val[npat * 9]   value of slot (c+1)*3 + (d+1) of every pattern (unused slots: anything)
 *   d_st_mask[npat]      bit s set = slot s present in the pattern
 *   union_mask           OR of all d_st_mask (slots nobody uses are never loaded)
 * (learnmultigrid_amd/ops.py StencilTwin.from_patterns derives line_stride and the table from a
 * verified RowPatterns twin and refuses everything else; at most lmg_stencil_limits patterns.)
 * A lane owns two consecutive rows, reads x with three 16-byte loads and shares the left / right
 * neighbours inside the wave -- 7 vector-memory instructions per 128 rows instead of 16-24 -- and
 * accumulates every row's entries in ascending column order: same modes, argument meaning and bits
 * as lmg_rpat_sweep.  d_x, d_b, d_out must be 16-byte aligned; square matrices only (x has n entries). */
int lmg_stencil_limits(int32_t *max_patterns);
int lmg_stencil_sweep(int mode, int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                      const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask, const double *d_x,
                      const double *d_b, double *d_out, double alpha, double beta, double *d_partials,
                      double *d_norm2, void *stream);

/* Fused smoothing pass on a grid-stencil matrix (same format arguments as lmg_stencil_sweep):
 *     x_out = J^sweeps(x_in),  J(x) = x + omega * D^-1 (b - A x),   sweeps = 1..3,
 *     r_out = b - A x_out      (d_r_out may be NULL),
 * i.e. the `smooth_steps` sweeps of Multigrid.py:88 / :121 and the residual of :90 in ONE pass over
 * x_in, b and the pattern ids (temporal blocking in registers: a wave marches down a 128-column strip
 * with all intermediate iterates in registers, see csrc/stencil_fused.hip).  d_x_in == NULL means a zero
 * initial iterate (coarse levels, Multigrid.py:103): the first sweep then is omega * (D^-1 b), the bits
 * of lmg_vmul.  hot_pattern / h_hot_val (HOST pointer to its 9 slot values; -1 / NULL: none) name a
 * pattern that has every slot of union_mask and a non-zero diagonal -- the interior row of a grid
 * operator: lines on which all lanes of a wave hold it run with its values in scalar registers.  Every
 * value equals the one the separate lmg_stencil_sweep launches produce, bit for bit.  x_out (and
 * r_out) must not alias x_in.  Compiled for the union masks lmg_stencil_smooth_supported accepts
 * (5-point 0x0BA, 9-point 0x1FF, 1-D 0x038); LMG_ERR_CAPACITY for others (run the separate sweeps). */
int lmg_stencil_smooth_supported(uint32_t union_mask);
int lmg_stencil_smooth(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                       const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                       int32_t hot_pattern, const double *h_hot_val, int sweeps, const double *d_x_in,
                       const double *d_b, double omega, double *d_x_out, double *d_r_out, void *stream);

/* The same pass for SMALL levels (10^4 .. 10^6 rows), iterates in LDS instead of registers: a workgroup owns a tile
 * of 64 columns x 16 / 32 lines, loads it once, runs the sweeps between two LDS buffers and stores its inner part
 * (csrc/stencil_tile.hip): one launch instead of sweeps + 1, same bits.  Same arguments as lmg_stencil_smooth;
 * 5- and 9-point union masks (lmg_stencil_smooth_tiled_supported). */
int lmg_stencil_smooth_tiled_supported(uint32_t union_mask);
int lmg_stencil_smooth_tiled(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                             const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                             int32_t hot_pattern, const double *h_hot_val, int sweeps, const double *d_x_in,
                             const double *d_b, double omega, double *d_x_out, double *d_r_out, void *stream);
/* ... and with the coarse-grid correction folded in, x_out = J^sweeps(x_in + P e_coarse): the tile is loaded as
 * x + P e (row patterns of P and the frequent pairs h_hot_pairs / h_hot_pval as in lmg_stencil_smooth_prolong, both
 * may be NULL; the correction is formed once per element, with the sums of lmg_rpat_sweep_grid(SPMV, alpha = 1,
 * beta = 1) in order). */
int lmg_stencil_smooth_tiled_prolong(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                                     const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                                     int32_t hot_pattern, const double *h_hot_val, int sweeps, const double *d_x_in,
                                     const double *d_b, double omega, double *d_x_out, int64_t n_coarse,
                                     int32_t coarse_stride, const double *d_e_coarse, const uint8_t *d_p_pid,
                                     int32_t p_npat, const double *d_p_val, const int32_t *d_p_mask,
                                     const int32_t *h_hot_pairs, const double *h_hot_pval, void *stream);
/* ... and with the restriction folded in, b_coarse = R (b - A x_out) instead of the residual (arguments of
 * lmg_stencil_smooth_restrict; hot_r: a pattern of R with all nine slots, -1 = none): the residual of the tile goes to
 * LDS, the row of R of every (even line, even column) node sums its nine entries in column order. */
int lmg_stencil_smooth_tiled_restrict(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                                      const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                                      int32_t hot_pattern, const double *h_hot_val, int sweeps, const double *d_x_in,
                                      const double *d_b, double omega, double *d_x_out, int64_t n_coarse,
                                      int32_t coarse_stride, double *d_b_coarse, const uint8_t *d_r_pid,
                                      int32_t r_npat, const double *d_r_val, const int32_t *d_r_mask, int32_t hot_r,
                                      const double *h_hot_rval, void *stream);
/* ... and both, the TURNAROUND of a repeated level visit (W- and F-cycles): the post-smoothing pass of visit k and the
 * pre-smoothing pass of visit k + 1 in one pass,
 *     x_out = J^(sweeps_post + sweeps_pre)(x_in + P e_coarse),   b_coarse = R (b - A x_out),
 * sweeps_post, sweeps_pre 1..3 each.  Arguments: the union of lmg_stencil_smooth_tiled_prolong's and
 * lmg_stencil_smooth_tiled_restrict's (one coarse grid: n_coarse, coarse_stride as the restriction demands); b_coarse
 * must not alias e_coarse.  Same bits as the correcting pass followed by the restricting pass; the halo is
 * sweeps_post + sweeps_pre + 2 lines and columns, the tile 64 columns x 32 or 64 lines (tune key tile_turnaround_rows). */
/* The tiled passes with ONE STEP OF THE CHEBYSHEV POLYNOMIAL SMOOTHER of degree 1..3 on D^-1 A in place of the Jacobi
 * sweeps: sweep k = 0 .. degree - 1 of the pass is
 *     d = a_k * d + c_k * (D^-1 (b - A x))   (k = 0: d = c_0 * (D^-1 (b - A x)), no add),     x = x + d,
 * h_coef = HOST pointer to (a_0, c_0, a_1, c_1, ..) -- 2 * degree doubles, handed to the kernel in scalar registers; d
 * lives in registers for the length of the pass and is never carried between launches.  Row sums in slot order, products
 * and sums rounded separately: degree 1 is lmg_stencil_smooth_tiled with omega = c_0 bit for bit, and every degree has
 * the bits of lmg_stencil_sweep(residual) + lmg_cheby_update per sweep.  Otherwise the arguments, rules and transfers of
 * lmg_stencil_smooth_tiled / _tiled_prolong / _tiled_restrict (there is no Chebyshev turnaround pass). */
int lmg_stencil_cheby_tiled(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                            const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                            int32_t hot_pattern, const double *h_hot_val, int degree, const double *h_coef,
                            const double *d_x_in, const double *d_b, double *d_x_out, double *d_r_out, void *stream);
int lmg_stencil_cheby_tiled_prolong(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                                    const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                                    int32_t hot_pattern, const double *h_hot_val, int degree, const double *h_coef,
                                    const double *d_x_in, const double *d_b, double *d_x_out, int64_t n_coarse,
                                    int32_t coarse_stride, const double *d_e_coarse, const uint8_t *d_p_pid,
                                    int32_t p_npat, const double *d_p_val, const int32_t *d_p_mask,
                                    const int32_t *h_hot_pairs, const double *h_hot_pval, void *stream);
int lmg_stencil_cheby_tiled_restrict(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                                     const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                                     int32_t hot_pattern, const double *h_hot_val, int degree, const double *h_coef,
                                     const double *d_x_in, const double *d_b, double *d_x_out, int64_t n_coarse,
                                     int32_t coarse_stride, double *d_b_coarse, const uint8_t *d_r_pid,
                                     int32_t r_npat, const double *d_r_val, const int32_t *d_r_mask, int32_t hot_r,
                                     const double *h_hot_rval, void *stream);
int lmg_stencil_smooth_tiled_turnaround(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                                        const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                                        int32_t hot_pattern, const double *h_hot_val, int sweeps_post, int sweeps_pre,
                                        const double *d_x_in, const double *d_b, double omega, double *d_x_out,
                                        int64_t n_coarse, int32_t coarse_stride, const double *d_e_coarse,
                                        const uint8_t *d_p_pid, int32_t p_npat, const double *d_p_val,
                                        const int32_t *d_p_mask, const int32_t *h_hot_pairs, const double *h_hot_pval,
                                        double *d_b_coarse, const uint8_t *d_r_pid, int32_t r_npat,
                                        const double *d_r_val, const int32_t *d_r_mask, int32_t hot_r,
                                        const double *h_hot_rval, void *stream);

/* ---- fused smoothing passes for grid operators with VARIABLE coefficients (csrc/dia_tile.hip) ------------------------
 * The operators the reference's learned transfers are built for (variable-coefficient / jittered-mesh stiffness
 * matrices, Multigrid.py:306-370, :741-765) have the 3x3 slot geometry of lmg_stencil_sweep -- every entry at
 * column - row = c * line_stride + d, c, d in {-1, 0, 1} -- but no repeating rows.  Their DIA twin stores one fp64 array
 * of n values per slot of the union mask, slots ascending: d_dia[q * n + row] (40 B/row for a 5-point operator; a row
 * without that slot holds +0.0, bitwise neutral for finite iterates like an explicit zero of the CSR input).
 *   lmg_dia_fill   : d_dia from sorted CSR; *d_mismatch |= 1 if an entry is no slot of the mask (d_dia = NULL: probe only,
 *                    the slots seen are OR-ed into *d_mask_out);
 *   lmg_dia_smooth : x_out = J^sweeps(x_in) (x_in = NULL: zero iterate), r_out = b - A x_out (optional), sweeps 1..3, in
 *                    ONE pass: the `sweeps` forward relaxations of pyamg's gauss_seidel call sites in their weighted-
 *                    Jacobi form (Multigrid.py:88, :121; Jacobi.py:35) plus the residual of :90 -- a workgroup per
 *                    64-column tile, the matrix values of a lane's rows in registers for all sweeps, the iterate in LDS;
 *                    same bits as lmg_csr_jacobi x sweeps + lmg_csr_residual_norm2.  Union masks: 5-point, both 7-point
 *                    orientations, 9-point (lmg_dia_smooth_supported). */
int lmg_dia_smooth_supported(uint32_t union_mask);
int lmg_dia_fill(int64_t n, int32_t line_stride, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                 uint32_t union_mask, double *d_dia, int32_t *d_mismatch, uint32_t *d_mask_out, void *stream);
int lmg_dia_smooth(int64_t n, int32_t line_stride, uint32_t union_mask, const double *d_dia, int sweeps,
                   const double *d_x_in, const double *d_b, double omega, double *d_x_out, double *d_r_out, void *stream);
/* ... and with one Chebyshev step of degree 1..3 in place of the Jacobi sweeps (h_coef and arithmetic of
 * lmg_stencil_cheby_tiled): same bits as lmg_csr_residual_norm2 + lmg_cheby_update per sweep. */
int lmg_dia_cheby(int64_t n, int32_t line_stride, uint32_t union_mask, const double *d_dia, int degree,
                  const double *h_coef, const double *d_x_in, const double *d_b, double *d_x_out, double *d_r_out,
                  void *stream);
/* The same three with fp32 slot arrays (a cycle used as a preconditioner: 4 B per slot and row).  The twin then IS the
 * matrix A32 = double(float(A)), value by value: a value is widened when it is loaded and everything after that -- products,
 * summation order, the diagonal -- is the fp64 pass, so the outputs have the bits of the fp64 entry points on a twin of A32.
 * Vectors and accumulation stay fp64.  lmg_dia_fill_f32 also raises bit 1 of *d_mismatch (|= 2) when a stored value other
 * than 0 is not finite or rounds to +-inf, a subnormal or zero: rounding must not change what an entry is, the caller then
 * keeps the fp64 twin.  Same argument checks and status codes as the fp64 forms. */
int lmg_dia_fill_f32(int64_t n, int32_t line_stride, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                     uint32_t union_mask, float *d_dia, int32_t *d_mismatch, uint32_t *d_mask_out, void *stream);
int lmg_dia_smooth_f32(int64_t n, int32_t line_stride, uint32_t union_mask, const float *d_dia, int sweeps,
                       const double *d_x_in, const double *d_b, double omega, double *d_x_out, double *d_r_out,
                       void *stream);
int lmg_dia_cheby_f32(int64_t n, int32_t line_stride, uint32_t union_mask, const float *d_dia, int degree,
                      const double *h_coef, const double *d_x_in, const double *d_b, double *d_x_out, double *d_r_out,
                      void *stream);

/* The same pass with the coarse-grid correction folded in (Multigrid.py:115 + :121 in one pass):
 *     x_out = J^sweeps(x_in + P e_coarse)
 * for a prolongation P whose row (y, x) -- y = row / line_stride, x = row % line_stride -- reads
 * e_coarse only at  ((y >> 1) * coarse_stride + (x >> 1)) + {0, 1, coarse_stride, coarse_stride + 1}  (slots
 * 0..3, ascending columns): the tensor-product interpolation between nested grids, stored as row
 * patterns (d_p_pid: one uint8 id per row of P; d_p_val [p_npat][4] values by slot, d_p_mask [p_npat]
 * slots present; rows on even lines must not use slots 2, 3).  x_in + P e is never written: the
 * correction is formed when a line arrives, with the sums of lmg_rpat_sweep_grid(SPMV, alpha = 1, beta = 1)
 * in the same order, so x_out has the bits of prolongation + separate sweeps.  h_hot_pairs (HOST, 2 ints,
 * may be NULL): for even / odd lines the ids (even column | odd column << 8) of the usual pattern pair,
 * with masks {0}, {0,1} / {0,2}, {0,1,2,3}, or -1; h_hot_pval (HOST, 9 doubles): their values in that
 * order.  5- and 9-point union masks (lmg_stencil_smooth_prolong_supported).
 * PRECONDITION (this entry point and lmg_stencil_smooth_restrict, not their _tiled forms): no entry of the operator
 * crosses the end of a line -- no pattern used in column 0 of a line has a slot of column - 1, none used in column
 * line_stride - 1 a slot of column + 1 (x-periodic operators, a 7-point operator read with the stride of its other
 * orientation).  A lane owns a coarse column here, so the elements beyond a line end, which only such an entry reads,
 * get the correction of the wrong coarse nodes.  The caller checks (ops.py: StencilTwin.line_end_coupling). */
int lmg_stencil_smooth_prolong_supported(uint32_t union_mask);
int lmg_stencil_smooth_prolong(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                               const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                               int32_t hot_pattern, const double *h_hot_val, int sweeps, const double *d_x_in,
                               const double *d_b, double omega, double *d_x_out, int64_t n_coarse,
                               int32_t coarse_stride, const double *d_e_coarse, const uint8_t *d_p_pid,
                               int32_t p_npat, const double *d_p_val, const int32_t *d_p_mask,
                               const int32_t *h_hot_pairs, const double *h_hot_pval, void *stream);

/* The pre-smoothing pass with the restriction folded in (Multigrid.py:88 + :90 + :93 in one pass):
 *     x_out = J^sweeps(x_in),   b_coarse = R (b - A x_out)
 * for a restriction R whose row (Y, X) -- Y = row / coarse_stride, X = row % coarse_stride -- reads the fine
 * residual only at  (2 Y * line_stride + 2 X) + c * line_stride + d,  c, d in {-1, 0, 1}  (slots 0..8,
 * ascending columns): the transpose of the tensor-product interpolation, stored as row patterns (d_r_pid:
 * one uint8 id per row of R; d_r_val [r_npat][9], d_r_mask [r_npat]).  The residual is never written: its last
 * three lines stay in registers, and every coarse row is summed like lmg_rpat_sweep_grid(SPMV, alpha = 1,
 * beta = 0) would, so b_coarse has the bits of residual + restriction launches.  Every fine node (even line,
 * even column) must have its coarse row (LMG_ERR_ARG otherwise).  hot_r / h_hot_rval (HOST, 9 doubles): a
 * pattern with all nine slots, or -1 / NULL.  d_x_in == NULL: zero initial iterate, as in lmg_stencil_smooth.
 * Precondition: no entry of the operator across the end of a line (see lmg_stencil_smooth_prolong). */
int lmg_stencil_smooth_restrict(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                                const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                                int32_t hot_pattern, const double *h_hot_val, int sweeps, const double *d_x_in,
                                const double *d_b, double omega, double *d_x_out, int64_t n_coarse,
                                int32_t coarse_stride, double *d_b_coarse, const uint8_t *d_r_pid,
                                int32_t r_npat, const double *d_r_val, const int32_t *d_r_mask, int32_t hot_r,
                                const double *h_hot_rval, void *stream);

/* Census of the rows that do NOT hold the expected pattern, for the three passes above.  On the benchmark's fine
 * level -- on any constant-coefficient grid level -- every row away from the boundary is the hot pattern of A, the
 * hot pair of P for its parities, the hot pattern of R.  Where that holds for everything a wave reads, the pass runs
 * a third, UNIFORM body that never loads or tests a pattern id (csrc/stencil_fused.hip); which waves those are is
 * read from a table built once per twin:
 *   lmg_pattern_census       d_table [lines + 1][cells + 1] int32, lines = ceil(n / line_stride), cells =
 *                            ceil(line_stride / 32): entry [y + 1][c + 1] = number of rows on the lines 0 .. y, columns
 *                            0 .. 32 c + 31 whose id differs from h_expected[2 * (line & 1) + (column & 1)] (HOST, 4 ints;
 *                            -1: nothing is expected there, every row counts), 2-D inclusive prefix sums behind a border
 *                            of zeros, so that a rectangle of cells is counted with four loads.  Columns of a cell beyond
 *                            the line stride and rows beyond n count as well.  Every entry is written.
 *   lmg_pattern_census_count its number of entries (0: arguments out of range).
 * The rules: A  all four = hot_pattern;  P  {pairs[0] & 255, pairs[0] >> 8, pairs[1] & 255, pairs[1] >> 8} of
 * h_hot_pairs;  R  all four = hot_r, over the COARSE grid (n_coarse, coarse_stride).
 * OWNERSHIP AND STALENESS: the caller owns the tables (learnmultigrid_amd/twins.py: each of StencilTwin, ProlongTwin,
 * RestrictTwin builds its own where it decides its hot ids, and holds it next to them).  A table is valid exactly as
 * long as the id array AND the hot ids it was built from: whoever writes or replaces either rebuilds or drops the table
 * with them, before the next launch.  A stale table makes the pass apply the hot values to rows that do not hold them.
 *   lmg_stencil_smooth*_census   the three passes with the tables: d_census (A), d_p_census (P), d_r_census (R), each NULL
 *                            = not given, and census_stride / r_census_stride = cells + 1 of the grid the table is
 *                            over (LMG_ERR_ARG otherwise).  A wave takes the UNIFORM body only where every table its
 *                            pass needs is given and zero over all it reads; same bits as the entry points above,
 *                            which take no tables and never run that body.  Only the kernels of THREE sweeps have the
 *                            body (not the plain pass from a zero iterate: it cost the others registers); with any other
 *                            sweep count the tables are accepted and not read.
 *   lmg_stencil_smooth_uniform_items   the kernels' own predicate on the host: h_counts[0..2] (HOST) = items (waves) of
 *                            the launch that run the general, the FAST and the UNIFORM body, for this geometry, the
 *                            tune keys as they stand and HOST copies of the tables.  form: 0 plain (with_residual,
 *                            zero_iterate as the launch), 1 correcting, 2 restricting (n_coarse, coarse_stride). */
int64_t lmg_pattern_census_count(int64_t n, int32_t line_stride);
int lmg_pattern_census(int64_t n, int32_t line_stride, const uint8_t *d_pid, const int32_t *h_expected, int32_t *d_table,
                       void *stream);
int lmg_stencil_smooth_census(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                              const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                              int32_t hot_pattern, const double *h_hot_val, int sweeps, const double *d_x_in,
                              const double *d_b, double omega, double *d_x_out, double *d_r_out,
                              const int32_t *d_census, int32_t census_stride, void *stream);
int lmg_stencil_smooth_prolong_census(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                                      const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                                      int32_t hot_pattern, const double *h_hot_val, int sweeps, const double *d_x_in,
                                      const double *d_b, double omega, double *d_x_out, int64_t n_coarse,
                                      int32_t coarse_stride, const double *d_e_coarse, const uint8_t *d_p_pid,
                                      int32_t p_npat, const double *d_p_val, const int32_t *d_p_mask,
                                      const int32_t *h_hot_pairs, const double *h_hot_pval, const int32_t *d_census,
                                      const int32_t *d_p_census, int32_t census_stride, void *stream);
int lmg_stencil_smooth_restrict_census(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                                       const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                                       int32_t hot_pattern, const double *h_hot_val, int sweeps, const double *d_x_in,
                                       const double *d_b, double omega, double *d_x_out, int64_t n_coarse,
                                       int32_t coarse_stride, double *d_b_coarse, const uint8_t *d_r_pid,
                                       int32_t r_npat, const double *d_r_val, const int32_t *d_r_mask, int32_t hot_r,
                                       const double *h_hot_rval, const int32_t *d_census, int32_t census_stride,
                                       const int32_t *d_r_census, int32_t r_census_stride, void *stream);
int lmg_stencil_smooth_uniform_items(int64_t n, int32_t line_stride, int sweeps, int with_residual, int zero_iterate,
                                     int form, int64_t n_coarse, int32_t coarse_stride, const int32_t *h_census,
                                     const int32_t *h_p_census, const int32_t *h_r_census, int64_t *h_counts);

/* ---- sliced-ELL ("SELL-64") sweeps: matrices with long rows ---------------------------
 * Third lossless twin.  Slice s = rows 64 s .. 64 s + 63, padded to its longest row
 * d_slice_len[s]; entry j of row r lives at d_slice_base[s] + 64 j + (r mod 64) of d_col
 * (colmode 0: uint16 column - d_slice_cmin[s]; 1: int32 column) and d_val (fp64), so a wave
 * reads entry j of its 64 rows with one coalesced load per stream and needs no LDS.  Rows are
 * still accumulated in storage order: same bits as the CSR entry points.  d_rowlen[n] = true
 * row lengths; max_len = longest row (picks the unrolling); modes and arguments as
 * lmg_pcsr_sweep.  Building: lmg_sell_slice_info (padded length and column range per slice),
 * d_slice_base = exclusive int64 scan of 64 * d_slice_len, lmg_sell_fill (d_col_out may be NULL
 * to refresh the values only); the padded arrays must be zero-initialised. */
int lmg_sell_sweep(int mode, int64_t n, const int64_t *d_slice_base, const int32_t *d_slice_len,
                   const int32_t *d_slice_cmin, const int32_t *d_rowlen, const void *d_col, int colmode,
                   const double *d_val, int32_t max_len, const double *d_x, const double *d_b, double *d_out,
                   double alpha, double beta, double *d_partials, double *d_norm2, void *stream);
int lmg_sell_slice_info(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, int32_t *d_slice_len,
                        int32_t *d_cmin, int32_t *d_cmax, void *stream);
int lmg_sell_fill(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                  const int64_t *d_slice_base, const int32_t *d_slice_cmin, int colmode, void *d_col_out,
                  double *d_val_out, void *stream);
/* ... and with an fp32 value stream (6 B per entry with uint16 columns): the twin is A32 = double(float(A)), a value is
 * widened when loaded, the rest is the fp64 sweep -- same bits as lmg_sell_sweep on a twin of A32.  lmg_sell_fill_f32 rounds
 * the values and sets *d_flag |= 1 (required, zeroed by the caller) when a stored value other than 0 is not finite or
 * rounds to +-inf, a subnormal or zero; the caller then keeps fp64 values.  Same checks and status codes otherwise. */
int lmg_sell_sweep_f32(int mode, int64_t n, const int64_t *d_slice_base, const int32_t *d_slice_len,
                       const int32_t *d_slice_cmin, const int32_t *d_rowlen, const void *d_col, int colmode,
                       const float *d_val, int32_t max_len, const double *d_x, const double *d_b, double *d_out,
                       double alpha, double beta, double *d_partials, double *d_norm2, void *stream);
int lmg_sell_fill_f32(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                      const int64_t *d_slice_base, const int32_t *d_slice_cmin, int colmode, void *d_col_out,
                      float *d_val_out, int32_t *d_flag, void *stream);

/* ---- the SELL sweeps on a block of k vectors: one pass over the matrix for k right-hand sides ----------------------------
 * Layout: a block of k vectors of length n is ONE contiguous fp64 array, X[i * k + j] = row i, column j (row-major,
 * interleaved), k = 2, 4 or 8 (LMG_ERR_ARG otherwise), base 16-byte aligned (LMG_ERR_ALIGN otherwise: d_X, d_B, d_Out).
 * lmg_sell_sweep_block: modes, SELL arguments (fp64 values only) and null rules of lmg_sell_sweep; d_X has k columns of the
 * matrix's column count, d_B and d_Out k columns of n rows.  An entry's column and value are loaded once, the k values of
 * its row of d_X as 16-byte loads.  No overlap: d_Out must not alias d_X (mode 1, Jacobi, and mode 2; LMG_ERR_ARG where
 * the bases are equal), the sweeps are not in place.  Summation order: column j accumulates its row in storage order
 * with separately rounded products, like lmg_sell_sweep -- the diagonal rule, diag == 0 -> out = x and the alpha / beta
 * special cases included --, so column j of d_Out carries the bits of lmg_sell_sweep run on column j alone.  A zero
 * column stays zero.  Mode 0: d_norm2[j] (k doubles) = sum of r_ij^2 over i, reduced per column over the same row -> lane
 * -> workgroup map and in the same order as lmg_sell_sweep's norm2; d_partials: lmg_block_partials_count(n, k) doubles of
 * scratch.  n == 0: LMG_OK, nothing is touched.  Every argument error is returned before any HIP call.
 * lmg_dense_gemv_block: Y = M X for a dense row-major n x m matrix and blocks X (m x k), Y (n x k): the coarsest-level
 * solve with the dense inverse, M read once for all k columns.  One wave per row; a lane adds the pairs (m even) or
 * elements (m odd) lmg_dense_gemv's one-wave-per-row kernel gives it, in its order, and the wave butterfly runs per column:
 * column j of Y has the bits of that kernel on column j.  d_M, d_X, d_Y 16-byte aligned; d_Y must not alias d_X. */
int64_t lmg_block_partials_count(int64_t n, int k);
int lmg_sell_sweep_block(int mode, int k, int64_t n, const int64_t *d_slice_base, const int32_t *d_slice_len,
                         const int32_t *d_slice_cmin, const int32_t *d_rowlen, const void *d_col, int colmode,
                         const double *d_val, int32_t max_len, const double *d_X, const double *d_B, double *d_Out,
                         double alpha, double beta, double *d_partials, double *d_norm2, void *stream);
int lmg_dense_gemv_block(int k, int64_t n, int64_t m, const double *d_M, const double *d_X, double *d_Y, void *stream);

/* ---- building the packed twin (setup) ----------------------------------------------
 * One streaming pass each; learnmultigrid_amd/ops.py PackedCSR.from_csr is the calling sequence.
 *   lmg_pcsr_tile_colrange   smallest / largest column of every tile of `tile_rows` rows
 *                            (0 / 0 for an empty tile)
 *   lmg_pcsr_encode_cols16   d_out[e] = uint16(d_colidx[e] - d_colbase[tile of e])
 *   lmg_value_set_insert     inserts the bit patterns of d_vals into an open-addressing table
 *                            (d_table: table_slots uint64, a power of two >= 2 * (limit + 262144),
 *                            pre-filled with 0xFF bytes).  d_state[3] (zeroed by the caller):
 *                            [0] distinct values seen, [1] != 0 if more than `limit` (the table
 *                            content is then meaningless), [2] != 0 if the all-ones pattern --
 *                            the empty marker -- occurs among the values.
 *   lmg_value_encode         d_out[e] = index of d_vals[e] in d_dict (width 1: uint8, 2: uint16);
 *                            d_dict sorted ascending as SIGNED 64-bit patterns; *d_missing is set
 *                            when a value is not in the dictionary.
 *   lmg_csr_inverse_diagonal d_dinv[i] = 1 / sum of the diagonal entries of row i, 0 when
 *                            that sum is 0 or the row has no diagonal entry. */
int lmg_pcsr_tile_colrange(int64_t n, int32_t tile_rows, const int32_t *d_rowptr, const int32_t *d_colidx,
                           int32_t *d_cmin, int32_t *d_cmax, void *stream);
int lmg_pcsr_encode_cols16(int64_t n, int32_t tile_rows, const int32_t *d_rowptr, const int32_t *d_colidx,
                           const int32_t *d_colbase, uint16_t *d_out, void *stream);
/* the occupied slots of that table, appended in ANY order to d_out (at most cap of them; *d_count, zeroed by the caller,
 * receives how many there were): the few survivors are sorted on the host */
int lmg_value_set_collect(const uint64_t *d_table, int64_t table_slots, uint64_t *d_out, int32_t cap, int32_t *d_count,
                          void *stream);
int lmg_value_set_insert(int64_t count, const double *d_vals, uint64_t *d_table, int64_t table_slots,
                         int32_t limit, int32_t *d_state, void *stream);
int lmg_value_encode(int64_t count, const double *d_vals, const double *d_dict, int32_t ndict, int width,
                     void *d_out, int32_t *d_missing, void *stream);
int lmg_csr_inverse_diagonal(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                             double *d_dinv, void *stream);

/* ---- Chebyshev polynomial smoother: the pieces outside the fused passes -------------------------------------------------
 *   lmg_cheby_update    one step after a residual launch of ANY format, in one pass at 16 B per lane:
 *                           d = a * d + c * (dinv * r)   (first != 0: d = c * (dinv * r), d is not read),   x = x + d
 *                       dinv from lmg_csr_inverse_diagonal; the vectors must be distinct and 16-byte aligned.
 *   lmg_csr_gershgorin  *d_lmax = max_i (sum_j |a_ij|) / |a_ii| over the rows with a non-zero diagonal (0 without any): the
 *                       Gershgorin bound of the spectrum of D^-1 A, never below its largest eigenvalue.  Row sums in
 *                       storage order, one maximum: bit-reproducible.  One memset and one launch (setup). */
int lmg_cheby_update(int64_t n, double a, double c, int first, const double *d_dinv, const double *d_r, double *d_d,
                     double *d_x, void *stream);
int lmg_csr_gershgorin(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals, double *d_lmax,
                       void *stream);

/* ---- line relaxation: the tridiagonal systems of the grid lines (csrc/line.hip) -----------------------------------------
 * A level of n rows with line stride W (n % line_stride == 0, LMG_ERR_ARG otherwise) has H = n / W lines.  dir 0 ("x"):
 * one system per storage line, rows k W .. k W + W - 1, its matrix T the entries of A at column - row in {-1, 0, +1};
 * dir 1 ("y"): one system per grid column k, rows k, k + W, k + 2 W, ..., the entries at column - row in {-W, 0, +W}.  A
 * missing entry is 0.  Lane <-> system in both kernels; products and sums round separately.
 *   lmg_line_factor  reads the tridiagonal part from the sorted, duplicate-free CSR and factors every system once: along
 *                    a system j = 0 .. L - 1 with sub-, main and super-diagonal lo_j, a_j, up_j,
 *                        den_0 = a_0,  den_j = a_j - lo_j * cp_(j-1),  minv_j = 1.0 / den_j,  cp_j = up_j * minv_j;
 *                    writes the three n-vectors d_lo, d_minv, d_cp (indexed by row; distinct), and ORs into *d_flags
 *                    (zeroed by the caller): bit 0 if, for dir 0, a stored non-zero entry couples two lines -- (i, i + 1)
 *                    with (i + 1) % W == 0, or (i + 1, i) --, bit 1 if a pivot den_j is zero or not finite.
 *   lmg_line_solve   x <- x + omega * T^-1 r on the systems first, first + step, ... (zebra: (0, 2) then (1, 2); all:
 *                    (0, 1)); every other row of d_x and d_r keeps its bits.  Forward  d_0 = r_0 * minv_0,
 *                    d_j = (r_j - lo_j * d_(j-1)) * minv_j  overwrites d_r; backward  e_(L-1) = d_(L-1),
 *                    e_j = d_j - cp_j * e_(j+1),  x_i = x_i + omega * e_j  updates d_x in place (the residual is formed
 *                    before the launch: no hazard).  No division, no scratch.  first < 0 or step < 1: LMG_ERR_ARG. */
int lmg_line_factor(int64_t n, int32_t line_stride, int dir, const int32_t *d_rowptr, const int32_t *d_colidx,
                    const double *d_vals, double *d_lo, double *d_minv, double *d_cp, int32_t *d_flags, void *stream);
int lmg_line_solve(int64_t n, int32_t line_stride, int dir, int64_t first, int64_t step, const double *d_lo,
                   const double *d_minv, const double *d_cp, double *d_r, double omega, double *d_x, void *stream);

/* The same for the wider lines of 25- and 49-point levels: band = p = 2 or 3 (anything else: LMG_ERR_ARG; p = 1 is the pair
 * above).  dir 0: the entries of A at column - row = m, |m| <= p, that stay inside the row's line -- one that leaves it
 * belongs to no system, and a non-zero one sets bit 0 of *d_flags --; dir 1: the entries at column - row = c W, |c| <= p.
 * Every other entry of a row is off-line coupling and is not looked at: the caller forms the true residual.
 * d_fac is one block of (2 p + 1) n doubles, 2 p + 1 planes of n doubles indexed by row:
 *     plane t - 1, t = 1 .. p   the multiplier l_(j,t) of row j for row j - t
 *     plane p                   minv_j = 1.0 / u_(j,0)
 *     plane p + q, q = 1 .. p   the upper entry u_(j,q), column j + q of row j of U
 * with j the row's place in its system.  Rows before the first and behind the last of a system count as zero rows.
 *   lmg_line_factor_banded  banded LU without pivoting, row by row: w = the band of row j; for t = p .. 1 (the rows
 *                    j - p .. j - 1 in that order)  l_(j,t) = w_(-t) * minv_(j-t),  then
 *                    w_(-t+q) = w_(-t+q) - l_(j,t) * u_(j-t,q)  for q = 1 .. p;  what is left of w is the upper row
 *                    u_(j,0..p), and minv_j = 1.0 / u_(j,0).  Bit 1 of *d_flags: a pivot u_(j,0) is zero or not finite.
 *                    d_fac must not be d_vals.  Two launches.
 *   lmg_line_solve_banded   x <- x + omega * (L U)^-1 r on the systems first, first + step, ...; every other row of d_x
 *                    and d_r keeps its bits.  Forward  s = r_j,  s = s - l_(j,t) * d_(j-t) for t = p .. 1,  d_j = s
 *                    overwrites d_r; backward  s = d_j,  s = s - u_(j,q) * e_(j+q) for q = p .. 1,  e_j = s * minv_j,
 *                    x_i = x_i + omega * e_j.  Products and sums round separately.  d_r and d_x must be distinct and
 *                    outside d_fac.  No division, no scratch. */
int lmg_line_factor_banded(int64_t n, int32_t line_stride, int dir, int band, const int32_t *d_rowptr,
                           const int32_t *d_colidx, const double *d_vals, double *d_fac, int32_t *d_flags, void *stream);
int lmg_line_solve_banded(int64_t n, int32_t line_stride, int dir, int band, int64_t first, int64_t step,
                          const double *d_fac, double *d_r, double omega, double *d_x, void *stream);

/* CSR transpose by counting sort (setup: the restriction R = P^T as an explicit CSR, `i.T` of
 * Multigrid.py:93).  lmg_csr_transpose_count: d_counts[c] (zeroed by the caller, ncols entries) += number of
 * entries in column c; the caller scans d_counts into d_t_rowptr with lmg_exclusive_scan_i32;
 * lmg_csr_transpose_fill places every entry (d_cursor: ncols zeroed int32) and sorts each row of A^T by
 * column, so the result equals SciPy's A.T.tocsr() for a sorted, duplicate-free A.  Rows of A^T longer than
 * lmg_csr_transpose_max_row() entries are sorted by a one-thread insertion sort too (slow): callers with
 * such rows use a library sort instead (ops.DeviceCSR.transpose does). */
int lmg_csr_transpose_max_row(void);
int lmg_csr_transpose_count(int64_t nnz, int64_t ncols, const int32_t *d_colidx, int32_t *d_counts, void *stream);
int lmg_csr_transpose_fill(int64_t n, int64_t ncols, const int32_t *d_rowptr, const int32_t *d_colidx,
                           const double *d_vals, const int32_t *d_t_rowptr, int32_t *d_cursor, int32_t *d_t_colidx,
                           double *d_t_vals, void *stream);

/* ---- Gauss-Seidel ---------------------------------------------------------------
 * One independent set: for every i in d_rows, in place,
 *     x_i = (b_i - sum_{j != i} a_ij x_j) / a_ii      (skipped when a_ii == 0)
 * -- the row update of pyamg's gauss_seidel (called at Multigrid.py:88,:121).  The rows
 * of one call must be mutually independent in the pattern of A + A^T. */
int lmg_csr_gs_rows(const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                    double *d_x, const double *d_b, const int32_t *d_rows, int64_t nrows,
                    void *stream);

/* `sweeps` sweeps over a schedule of `nsets` independent sets executed in order
 * (level schedule => exact lexicographic forward Gauss-Seidel; colour classes =>
 * multicolour Gauss-Seidel).  d_set_ptr / h_set_ptr are the same nsets+1 offsets into
 * d_set_rows on device and host.  max_set = largest set size. */
int lmg_csr_gs_schedule(const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                        double *d_x, const double *d_b, const int32_t *d_set_rows,
                        const int32_t *d_set_ptr, const int32_t *h_set_ptr, int64_t nsets,
                        int64_t max_set, int sweeps, void *stream);
/* The one-workgroup executor of lmg_csr_gs_schedule on a copy of the PATTERN in schedule order
 * (for schedules of a few thousand rows per set at most: grids up to ~1025^2): d_ell_row[k] the
 * k-th scheduled row, d_ell_start[k] / d_ell_len[k] its entry range in the CSR arrays,
 * d_ell_cols[j * total_rows + k] its j-th column (j < ell_k in {3, 5, 7, 9, 16} >= the longest
 * row; padding entries hold the row itself).  Values are read from d_vals, so the copy stays
 * valid across coefficient changes.  n = length of d_x (up to 18 000 unknowns the iterate is kept
 * in LDS for the whole call).  Same results as lmg_csr_gs_schedule, bit for bit. */
int lmg_csr_gs_schedule_ell(int64_t n, const double *d_vals, double *d_x, const double *d_b, const int32_t *d_ell_row,
                            const int32_t *d_ell_start, const int32_t *d_ell_len, const int32_t *d_ell_cols,
                            int32_t ell_k, int64_t total_rows, const int32_t *d_set_ptr, int64_t nsets,
                            int sweeps, void *stream);

/* Exact forward (lexicographic) Gauss-Seidel on a grid-stencil matrix (format arguments of
 * lmg_stencil_sweep) as a pipelined wavefront in registers: a wave owns 64 grid lines, lane l relaxes
 * column t - SK*l of its line at step t, neighbouring bands hand their boundary line over through memory
 * behind a progress counter (csrc/gs_wave.hip).  `sweeps` forward sweeps in place on d_x: the same bits as
 * lmg_csr_gs_schedule on the level schedule and as pyamg's gauss_seidel (Multigrid.py:88, :121), at ~0.15 us
 * per dependent anti-diagonal instead of a kernel launch each.  Requirements (the caller checks them:
 * ops.StencilTwin.gs_ok): union_mask accepted by lmg_stencil_gs_supported (5-, 7-, 9-point, 1-D), and no
 * pattern used in column 0 / line_stride-1 of a line couples across the line end.  hot_pattern /
 * h_hot_val as in lmg_stencil_smooth (steps in which every lane relaxes that pattern skip the LDS table).  d_work:
 * lmg_stencil_gs_work_bytes(n, line_stride) bytes, 8-byte aligned, its FIRST int32 zeroed by the caller
 * once (it is set when a band had to give up waiting: the result is then invalid).  Up to four sweeps share
 * one launch, pipelined behind each other (band b of sweep s trails band b + 1 of sweep s - 1), so the
 * pipeline fill -- 64 SK steps per band -- is paid once per launch, not once per sweep. */
int lmg_stencil_gs_supported(uint32_t union_mask);
int64_t lmg_stencil_gs_work_bytes(int64_t n, int32_t line_stride);
int lmg_stencil_gs_sweep(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                         const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                         int32_t hot_pattern, const double *h_hot_val, double *d_x, const double *d_b,
                         void *d_work, int sweeps, void *stream);
/* Exact BACKWARD Gauss-Seidel (rows n-1 .. 0; pyamg's gauss_seidel with sweep='backward'): the same arguments and
 * requirements as lmg_stencil_gs_sweep, plus n % line_stride == 0 (LMG_ERR_ARG otherwise; ragged grids take a reversed
 * level schedule).  The kernels of lmg_stencil_gs_sweep run in mirrored coordinates (row (y, x) -> (lines-1-y, W-1-x)),
 * so row (y, x) reads the NEW values of (y+1, x-1 .. x+1) and (y, x+1); rsum still runs over the entries in ascending
 * column order, then (b - rsum) / diag, rows with a zero diagonal untouched: the same bits as lmg_csr_gs_schedule on
 * the reversed level schedule.  Both directions use the operator's one d_work buffer (its tickets and progress
 * counters are reset by every launch): all sweeps on one operator, forward or backward, must stay ordered on ONE
 * stream.  The gsw_* tune keys apply to both directions. */
int lmg_stencil_gs_sweep_backward(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t npat,
                                  const double *d_st_val, const int32_t *d_st_mask, uint32_t union_mask,
                                  int32_t hot_pattern, const double *h_hot_val, double *d_x, const double *d_b,
                                  void *d_work, int sweeps, void *stream);

/* HOST helpers (host pointers, run on the CPU at setup time).
 * level[i] = 1 + max(level[j] : j < i adjacent to i in A + A^T), 0 if none: rows of equal
 * level are independent, executing levels in order IS the lexicographic sweep.
 * Returns the number of levels (>= 0) or a negative lmg_status. */
int64_t lmg_host_gs_levels(int64_t n, const int32_t *h_rowptr, const int32_t *h_colidx,
                           int32_t *h_level_out);
/* Greedy natural-order colouring of A + A^T; returns the number of colours. */
int64_t lmg_host_greedy_colors(int64_t n, const int32_t *h_rowptr, const int32_t *h_colidx,
                               int32_t *h_color_out);
/* The C/F split of NeuralMG_2D.coarsening (Multigrid.py:401-426, which walks a dense n x n copy of the mass matrix
 * and rebuilds Python sets per node): node i is coarse iff no coarse c < i has A[c][i] > 0 -- row c, so an unsymmetric
 * pattern is taken as it stands.  The lexicographically first maximal independent set, sequential, O(nnz).
 * h_is_coarse_out[i] = 1 | 0; returns the number of coarse nodes or a negative lmg_status. */
int64_t lmg_host_greedy_cf(int64_t n, const int32_t *h_rowptr, const int32_t *h_colidx, const double *h_vals,
                           int32_t *h_is_coarse_out);

/* ---- vectors --------------------------------------------------------------------*/
int lmg_axpby(int64_t n, double alpha, const double *d_x, double beta, double *d_y, void *stream);
/* out = alpha * (x * y) elementwise.  With x = 1/diag(A), y = b, alpha = omega this is the
 * Jacobi sweep from a zero initial guess (coarse levels start from zeros, Multigrid.py:103). */
int lmg_vmul(int64_t n, double alpha, const double *d_x, const double *d_y, double *d_out, void *stream);
int lmg_copy(int64_t n, const double *d_src, double *d_dst, void *stream);
int lmg_zero(int64_t n, double *d_x, void *stream);
int lmg_dot(int64_t n, const double *d_x, const double *d_y, double *d_partials, double *d_out,
            void *stream);
/* buf[k] = x[idx[k]] (halo pack) and x[idx[k]] = buf[k] (unpack). */
int lmg_gather(int64_t n, const int32_t *d_idx, const double *d_x, double *d_buf, void *stream);
int lmg_scatter(int64_t n, const int32_t *d_idx, const double *d_buf, double *d_x, void *stream);

/* ---- fused Gram-Schmidt passes of the Krylov solvers (csrc/krylov.hip) ----------------------------------------------------
 * A basis is a row-major block d_V[k][ldv] of doubles, ldv >= n and even, so that every row is 16-byte aligned like the
 * base (LMG_ERR_ARG for an odd ldv or ldv < n, LMG_ERR_ALIGN for a base of d_V or d_w off 16 bytes).  Elements n .. ldv-1
 * of a row, and rows >= k, are never read or written.  k <= lmg_krylov_max_vectors() (65: restart <= 64), LMG_ERR_ARG for
 * k < 0 or beyond.  d_partials: lmg_multi_partials_count(n, k) doubles of scratch for either call.
 *
 *   lmg_multi_dot    d_out[j] = V_j . w, j < k.  w is read once per 16 columns, every V_j once.
 *   lmg_multi_axpy   every element:  w = w - coef[0] * v_0,  then  - coef[1] * v_1, ... j ascending (subtract == 0: +); each
 *                    product and each sum rounds on its own, the bits of the loop `for j: w = w - coef[j] * V[j]`.
 *                    d_coef is a DEVICE array, typically the d_out of the lmg_multi_dot before it on the same stream.
 *                    d_norm2 != NULL receives |w_new|^2 (d_partials needed); NULL: no reduction, d_partials may be NULL
 *                    and is not written.  w is read and written once, every V_j read once.  w must not overlap d_V.
 *
 * Summation order, the same for every column and for |w|^2, independent of k, of the other columns and of every tune key:
 * 1024 workgroups of 256 lanes; lane t of workgroup g owns the element pairs (2 i, 2 i + 1), i = 256 g + t + 262144 m,
 * m = 0, 1, ..., and adds their products to one accumulator in ascending i, first element of the pair first; the last
 * element of an odd n is added by lane 0 of workgroup 0 after its pairs.  A workgroup's sum: 64-lane butterfly
 * (offsets 32, 16, ... 1), then its four waves in ascending order.  The 1024 partials: a second launch, one partial per
 * lane, butterfly, then the 16 waves in ascending order.  (Not the element <-> lane map of lmg_dot, which loads 8 bytes.)
 * k == 0 is LMG_OK (lmg_multi_axpy with d_norm2 then still sums |w|^2); n == 0 is LMG_OK, d_out[j] = 0 resp. *d_norm2 = 0. */
int lmg_krylov_max_vectors(void);
int64_t lmg_multi_partials_count(int64_t n, int k);
int lmg_multi_dot(int64_t n, int k, const double *d_V, int64_t ldv, const double *d_w, double *d_partials, double *d_out,
                  void *stream);
int lmg_multi_axpy(int64_t n, int k, int subtract, const double *d_V, int64_t ldv, const double *d_coef, double *d_w,
                   double *d_partials, double *d_norm2, void *stream);

/* ---- conjugate gradients on a block of k right-hand sides (csrc/krylov.hip) ------------------------------------------------
 * Blocks as in lmg_sell_sweep_block: X[i * k + j] = row i, column j, k = 2, 4 or 8 (LMG_ERR_ARG otherwise), base 16-byte
 * aligned (LMG_ERR_ALIGN otherwise).  Per-column scalars are DEVICE arrays of k doubles; the mask holds 1.0 for a column
 * that still iterates and 0.0 for one that is frozen (padding, converged).  No atomics, fixed geometry: nothing depends on
 * n, k or a tune key.  n == 0: LMG_OK, nothing is touched.  Every argument error is returned before any HIP call.
 *
 *   lmg_block_dot           d_out[j] = sum_i X[i,j] * Y[i,j], the k columns in one pass (d_X == d_Y allowed).  Column j has
 *                           the BITS of lmg_dot on a contiguous copy of column j: 1024 workgroups of 256 lanes, lane t of
 *                           workgroup g owns rows 256 g + t + 262144 m, m = 0, 1, ..., one accumulator per lane and column,
 *                           acc = acc + x * y in ascending rows; the workgroup's sum is a 64-lane butterfly, then its four
 *                           waves in ascending order; the 1024 partials of a column: one per lane of a second launch,
 *                           butterfly, then the 16 waves.  d_partials: lmg_block_dot_partials_count(n, k) doubles.
 *   lmg_block_cg_step       alpha_j = rz_j / pAp_j, one division, 0 where mask_j == 0 or pAp_j == 0.  For the columns
 *                           with mask_j != 0:  x = alpha p + x,  r = (-alpha) ap + r,  product and sum rounded on their own:
 *                           the bits of lmg_axpby(alpha, p, 1, x) and lmg_axpby(-alpha, ap, 1, r).  A column with
 *                           mask_j == 0 is not stored: its bytes of d_X and d_R stay as they are, whatever d_P and
 *                           d_AP hold there (NaN included).
 *                           d_rr[j] = sum_i r_ij^2 of d_R as it is afterwards, every column, the bits of lmg_block_dot(R, R).
 *                           The small second launch that sums the partials also sets
 *                           mask_j = (mask_j != 0 && rr_j > tol2_j) ? 1 : 0.
 *                           LMG_ERR_ARG where d_X, d_R, d_P, d_AP are not four different arrays, or d_rr is one of the
 *                           other scalar arrays.
 *   lmg_block_cg_direction  beta_j = rz_new_j / rz_old_j;  p = z + beta p for the columns with mask_j != 0, the bits of
 *                           lmg_axpby(1, z, beta, p) (beta_j == 0: p = z);  the others are not stored.  LMG_ERR_ARG for
 *                           d_P == d_Z or d_rz_new == d_rz_old: the driver alternates between two arrays, so no launch
 *                           writes a scalar that another workgroup of the same launch reads. */
int64_t lmg_block_dot_partials_count(int64_t n, int k);
int lmg_block_dot(int k, int64_t n, const double *d_X, const double *d_Y, double *d_partials, double *d_out, void *stream);
int lmg_block_cg_step(int k, int64_t n, const double *d_rz, const double *d_pAp, const double *d_tol2, double *d_mask,
                      const double *d_P, const double *d_AP, double *d_X, double *d_R, double *d_partials, double *d_rr,
                      void *stream);
int lmg_block_cg_direction(int k, int64_t n, const double *d_rz_new, const double *d_rz_old, const double *d_mask,
                           const double *d_Z, double *d_P, void *stream);

/* ---- flexible GMRES on a block of k right-hand sides (csrc/krylov.hip) -----------------------------------------------------
 * The Gram-Schmidt passes above on blocks: X[i * k + j] = row i, column j, k = 2, 4 or 8 (LMG_ERR_ARG otherwise), base
 * 16-byte aligned (LMG_ERR_ALIGN otherwise).  A block basis is nb such blocks, block i at d_V + i * ldb doubles, ldb >= n * k
 * and even (LMG_ERR_ARG otherwise); the doubles n * k .. ldb-1 of a block, and the blocks >= nb, are never read or written.
 * nb and every count are 0 .. lmg_krylov_max_vectors() (LMG_ERR_ARG beyond).  Null pointers: LMG_ERR_ARG.  No atomics, fixed
 * geometry.  nb == 0 and n == 0 are LMG_OK as for lmg_multi_*: d_out resp. d_norm2 are zeroed for n == 0.
 *
 *   lmg_block_multi_dot     d_out[i * k + j] = V_i[:, j] . W[:, j], i < nb, j < k, in one pass, with the BITS lmg_multi_dot
 *                           returns for row i when column j of every block and of W is copied into a contiguous basis:
 *                           1024 workgroups of 256 lanes, lane t of workgroup g owns the row pairs 256 g + t + 262144 m,
 *                           one accumulator per (i, j) and lane, row 2 p before row 2 p + 1, the last row of an odd n to
 *                           lane 0 of workgroup 0 after its pairs; then the sums of lmg_multi_dot (butterfly, four waves,
 *                           second launch over the 1024 partials).  A row pair of a block is 2 k contiguous doubles: k
 *                           16-byte loads per lane and block.  The blocks go through the registers 32 / k at a time
 *                           (16, 8, 4 for k = 2, 4, 8): W is read ceil(nb k / 32) times, every V_i once.
 *                           d_partials: lmg_block_multi_partials_count(n, k, nb) doubles.
 *   lmg_block_multi_axpy    column j:  w = w - coef[i * k + j] * V_i[:, j]  for i = 0 .. h_counts[j] - 1 ascending
 *                           (subtract == 0: +), every product and every sum rounded on its own: the bits of lmg_multi_axpy
 *                           with k = h_counts[j] on contiguous copies.  h_counts is a HOST array of k ints, read before the
 *                           call returns; d_coef is a DEVICE array in the layout of lmg_block_multi_dot's d_out, of
 *                           max_j h_counts[j] * k doubles.  A column with h_counts[j] == 0 is neither computed nor stored:
 *                           its bytes of d_W stay as they are (a pair of columns is one 16-byte store where both are on,
 *                           8 bytes where one is).  d_norm2 != NULL: d_norm2[j] = |W[:, j]|^2 as W stands afterwards, for
 *                           every column whatever its count, the bits of lmg_multi_axpy's folded norm on that column
 *                           (d_partials needed: lmg_block_multi_partials_count(n, k, 1) doubles); NULL: no reduction.
 *                           W is read and written once, V_0 .. V_(max count - 1) once.  d_W must not overlap the basis.
 *   lmg_block_scale         W[:, j] = h_scale[j] * W[:, j], the bits of lmg_axpby(h_scale[j], w, 0, w) on the column.
 *                           h_scale is a HOST array of k doubles, read before the call returns.  h_scale[j] == 0.0 stores
 *                           +0.0 whatever the column held, NaN and Inf included: how a column that has left a cycle is
 *                           emptied. */
int64_t lmg_block_multi_partials_count(int64_t n, int k, int nb);
int lmg_block_multi_dot(int k, int64_t n, int nb, const double *d_V, int64_t ldb, const double *d_W, double *d_partials,
                        double *d_out, void *stream);
int lmg_block_multi_axpy(int k, int64_t n, const int *h_counts, int subtract, const double *d_V, int64_t ldb, const double *d_coef,
                         double *d_W, double *d_partials, double *d_norm2, void *stream);
int lmg_block_scale(int k, int64_t n, const double *h_scale, double *d_W, void *stream);

/* ---- the two inner Krylov steps of a K-cycle visit (csrc/krylov.hip) -------------------------------------------------------
 * On a level of n rows with operator A, c1 and c2 the results of the two child visits, v1 = A c1, v2 = A c2, b the right-hand
 * side of the level.  gcr != 0: p = v (GCR, any A); gcr == 0: p = c (flexible CG, symmetric positive definite A and cycle).
 *
 *   lmg_kcycle_step1   alpha1 = <p1, b>, rho1 = <p1, v1>, t1 = rho1 != 0 ? alpha1 / rho1 : 0, rt = b + (-t1) * v1.
 *   lmg_kcycle_step2   gamma = <p2, v1>, beta = <p2, v2>, alpha2 = <p2, rt>;  rho1 and t1 are READ from d_scal;
 *                      q = rho1 != 0 ? gamma / rho1 : 0, rho2 = beta - gamma * q, t2 = rho2 != 0 ? alpha2 / rho2 : 0,
 *                      a = t1 - q * t2, x_out = a * c1 + t2 * c2.
 *
 * Every product and every sum is rounded on its own in the order written; non-finite values are not masked (NaN != 0).
 * d_scal: LMG_KC_SCALARS doubles on the DEVICE at the indices below, written by the device only (step 1 writes 0 .. 2, step 2
 * writes 3 .. 8).  Inputs are never written and nothing beyond element n - 1 is touched.  d_x_out may be d_c2 (same bits as
 * a separate output); an output that is any other input of its step is LMG_ERR_ARG.  Null pointers, n < 1, a form outside
 * 0 .. 2 and partials_count < lmg_kcycle_partials_count(n) are LMG_ERR_ARG, a vector off 16 bytes is LMG_ERR_ALIGN, all
 * before any launch.  d_partials: partials_count doubles of scratch.  With gcr != 0 step 1 does not read d_c1.
 *
 * Launches.  G = lmg_kcycle_grid(n) = min(ceil(n / 2048), 512) workgroups of 256 lanes, a function of n alone.  Lane t of
 * workgroup g owns the element pairs (2 i, 2 i + 1), i = 256 g + t + 256 G m, m = 0, 1, ..., one 16-byte load per vector
 * and step, one accumulator per product, first element of the pair first; the last element of an odd n goes to lane 0 of
 * workgroup 0 after its pairs.  A workgroup's share of a product: 64-lane butterfly, then its four waves in ascending order.
 * A product: lane t adds share t and share t + 256 (0.0 for a share >= G), butterfly, four waves.  No atomics.
 *   form 2 (two launches): the first writes one share per workgroup and product; in the second every workgroup sums the
 *          shares itself, forms the coefficients and updates its pairs; workgroup 0 writes d_scal.
 *   form 1 (one launch): one workgroup of 1024 lanes computes the G shares -- four at a time, quarter w of the workgroup
 *          being workgroup 4 m + w of form 2 -- keeps them in LDS, and goes on as every workgroup of the second launch.
 *   form 0: form 1 for n <= lmg_kcycle_one_launch_max(), else form 2.
 * The bits of d_rt, d_x_out and d_scal depend on the inputs and n only: not on the form, a tune key or the call history. */
enum {
    LMG_KC_ALPHA1 = 0,
    LMG_KC_RHO1 = 1,
    LMG_KC_T1 = 2,
    LMG_KC_GAMMA = 3,
    LMG_KC_BETA = 4,
    LMG_KC_ALPHA2 = 5,
    LMG_KC_RHO2 = 6,
    LMG_KC_T2 = 7,
    LMG_KC_A = 8,
    LMG_KC_SCALARS = 9
};
int lmg_kcycle_grid(int64_t n);
int64_t lmg_kcycle_partials_count(int64_t n);
int64_t lmg_kcycle_one_launch_max(void);
int lmg_kcycle_step1(int64_t n, int gcr, int form, const double *d_c1, const double *d_v1, const double *d_b, double *d_rt,
                     double *d_scal, double *d_partials, int64_t partials_count, void *stream);
int lmg_kcycle_step2(int64_t n, int gcr, int form, const double *d_c1, const double *d_v1, const double *d_c2,
                     const double *d_v2, const double *d_rt, double *d_scal, double *d_x_out, double *d_partials,
                     int64_t partials_count, void *stream);

/* ---- coarsest level --------------------------------------------------------------
 * y = M x for a dense row-major n x m matrix: applies a pre-factored coarse operator
 * (M = A_L^-1 computed once at setup) in place of the per-cycle SuperLU
 * `spsolve(A_coarse, res_coarse)` of Multigrid.py:106. */
int lmg_dense_gemv(int64_t n, int64_t m, const double *d_M, const double *d_x, double *d_y,
                   void *stream);
/* y_b = M_b x_b for nblocks dense bs x bs blocks stored one after the other (bs even):
 * the strip solves of the banded block-elimination coarse solver (coarse.py). */
int lmg_dense_gemv_blockdiag(int64_t nblocks, int64_t bs, const double *d_M, const double *d_x,
                             double *d_y, void *stream);

/* Batched GEMV on windows of a vector, for block k < nblocks and row r < rows:
 *     y[k*y_stride + r] = (d_z ? d_z[k*z_stride + r] : 0) + alpha * sum_c M[k][r][c] * x[k*x_stride + c]
 * (M: nblocks dense rows x cols blocks, row-major; windows may overlap).  The building block of the
 * block-cyclic-reduction coarse solver (coarse.py), which lifts the size limit of the dense / one-level
 * banded solvers: `spsolve` on coarse operators of 10^5 unknowns (2-level runs, Multigrid.py:106).
 * cols and x_stride even, M and x 16-byte aligned.  lmg_block_copy: dst[k*dst_stride + i] =
 * src[k*src_stride + i], i < bs. */
int lmg_dense_gemv_windows(int64_t nblocks, int64_t rows, int64_t cols, const double *d_M, const double *d_x,
                           int64_t x_stride, const double *d_z, int64_t z_stride, double alpha, double *d_y,
                           int64_t y_stride, void *stream);

/* The same with a table of window starts: the x window of block k is d_x[d_x_offsets[k] .. + cols) (any 8-byte
 * aligned start; the caller keeps every window inside the allocation).  Back-substitution of the banded coarse
 * solver: x_I = y_I - (A_II^-1 A_IS) x_S in one launch (coarse.py BandedBlockSolver.apply).  With
 * d_x_offsets[k] = k * x_stride the bits of lmg_dense_gemv_windows (one routine sums the rows of both). */
int lmg_dense_gemv_windows_off(int64_t nblocks, int64_t rows, int64_t cols, const double *d_M, const double *d_x,
                               const int32_t *d_x_offsets, const double *d_z, int64_t z_stride, double alpha,
                               double *d_y, int64_t y_stride, void *stream);

/* First and last product of the banded coarse solver (coarse.py) with its permutation perm = [strip unknowns |
 * separator unknowns] folded in, so that no gather / scatter launch surrounds the solve:
 *   lmg_coarse_front: y = blockdiag(M) b[perm[0 .. nblocks*bs)],  tail_out[i] = b[perm[nblocks*bs + i]], i < ntail;
 *   lmg_coarse_back : out[perm[k*rows + r]] (+)= z[k*z_stride + r] + alpha * M_k[r,:] . x[x_offsets[k] ..),
 *                     out[perm[nblocks*rows + i]] (+)= x[i], i < ntail   (accumulate != 0: += , the refinement step).
 * Every block of d_perm[0 .. nblocks*bs) is a run of consecutive indices (perm[k bs + c] = perm[k bs] + c: a strip of the
 * banded solver), which lmg_coarse_front relies on.
 * Same sums as lmg_dense_gemv_blockdiag / lmg_dense_gemv_windows_off followed by lmg_gather / lmg_scatter / lmg_axpby:
 * all of them sum a row through one routine (csrc/dense.hip). */
int lmg_coarse_front(int64_t nblocks, int64_t bs, const double *d_M, const double *d_b, const int32_t *d_perm, double *d_y,
                     int64_t ntail, double *d_tail_out, void *stream);
int lmg_coarse_back(int64_t nblocks, int64_t rows, int64_t cols, const double *d_M, const double *d_x,
                    const int32_t *d_x_offsets, const double *d_z, int64_t z_stride, double alpha, const int32_t *d_perm,
                    double *d_out, int accumulate, int64_t ntail, void *stream);

/* The same two products for blocks that are not runs of consecutive unknowns (coarse.py GridBlockSolver: rectangular
 * blocks of a grid cut by separator lines AND columns, padded to one size) -- every operand index comes from a table:
 *   lmg_coarse_front_gather: y[k*bs + r] = sum_c M_k[r][c] * b[d_idx[k*bs + c]]  (d_idx < 0: padding, contributes 0),
 *                            tail_out[i] = b[d_tail_idx[i]], i < ntail;
 *   lmg_coarse_back_gather : out[d_oidx[k*rows + r]] (+)= z[k*z_stride + r] + alpha * sum_c M_k[r][c] * x[d_xidx[k*cols + c]]
 *                            (d_oidx < 0: padding row, skipped),  out[d_tail_idx[i]] (+)= x[i], i < ntail.
 * bs and cols even, index tables 8-byte aligned.  Replaces the per-cycle SuperLU `spsolve` of Multigrid.py:106 together
 * with lmg_csr_spmv and lmg_dense_gemv (four launches per application). */
int lmg_coarse_front_gather(int64_t nblocks, int64_t bs, const double *d_M, const double *d_b, const int32_t *d_idx,
                            double *d_y, int64_t ntail, const int32_t *d_tail_idx, double *d_tail_out, void *stream);
int lmg_coarse_back_gather(int64_t nblocks, int64_t rows, int64_t cols, const double *d_M, const double *d_x,
                           const int32_t *d_xidx, const double *d_z, int64_t z_stride, double alpha, const int32_t *d_oidx,
                           double *d_out, int accumulate, int64_t ntail, const int32_t *d_tail_idx, void *stream);

/* Dense fp64 helpers of the coarse-solver SETUP (csrc/gemm.hip; what NumPy / SuperLU do on the host inside the reference's
 * per-cycle `spsolve`, Multigrid.py:106, is a one-off factorisation here): row-major, leading dimensions, batch strides.
 *   lmg_batched_gemm: C[b] = alpha * A[b] (M x K) * B[b] (K x N) + beta * C[b]   (beta == 0: C is not read)
 *   lmg_copy2d      : dst[b][r][c] = alpha * src[b][r][c]   (accumulate != 0: += ) */
int lmg_batched_gemm(int64_t batch, int64_t M, int64_t N, int64_t K, double alpha, const double *d_A, int64_t lda,
                     int64_t stride_a, const double *d_B, int64_t ldb, int64_t stride_b, double beta, double *d_C,
                     int64_t ldc, int64_t stride_c, void *stream);
int lmg_copy2d(int64_t batch, int64_t rows, int64_t cols, double alpha, const double *d_src, int64_t ld_src,
               int64_t stride_src, double *d_dst, int64_t ld_dst, int64_t stride_dst, int accumulate, void *stream);

/* Setup helper: d_counts[((y & 1) * 2 + (x & 1)) * 256 + id] += number of rows i = y * line_stride + x with pattern id
 * d_pid[i] = id (d_counts: 1024 int32, zeroed by the caller). */
int lmg_pattern_parity_counts(int64_t n, int32_t line_stride, const uint8_t *d_pid, int32_t *d_counts, void *stream);
int lmg_block_copy(int64_t nblocks, int64_t bs, const double *d_src, int64_t src_stride, double *d_dst,
                   int64_t dst_stride, void *stream);

/* Inverses of nmat dense n x n matrices (n <= 128, row-major, one after the other): one workgroup per
 * matrix, Gauss-Jordan with partial pivoting in LDS.  d_info[k] = 1 when matrix k has an exactly zero
 * pivot (d_Ainv of that matrix is then undefined).  Setup-time helper of the coarse solvers. */
/* d_dense (n x m, row-major, zeroed by the caller) += the CSR matrix (duplicate entries are summed). */
int lmg_csr_to_dense(int64_t n, int64_t m, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                     double *d_dense, void *stream);
int lmg_batched_inverse(int64_t nmat, int32_t n, const double *d_A, double *d_Ainv, int32_t *d_info, void *stream);

/* ---- Galerkin product (SpGEMM)  C = A * B -----------------------------------------
 * Replaces SciPy's csr_matmat behind `i.T @ A @ i` (Multigrid.py:97-98), evaluated as
 * (R A) P like SciPy does.  Row-wise Gustavson with an expand / stable-sort / in-order
 * compress per row, so C has sorted rows and every c_ik is accumulated in the order of
 * the products a_ij*b_jk as SciPy traverses them.
 *   1. lmg_spgemm_count     : d_row_products[i] = sum_j nnz(B_j)  (upper bound of nnz(C_i))
 *   2. lmg_spgemm_symbolic  : d_c_rownnz[i] = nnz(C_i)            (needs step 1)
 *      -- caller turns d_c_rownnz into d_c_rowptr with lmg_exclusive_scan_i32 --
 *   3. lmg_spgemm_numeric   : fills d_c_colidx / d_c_vals.
 * Rows whose product count exceeds LMG_SPGEMM_MAX_ROW_PRODUCTS are skipped by steps 2 and 3
 * and must be handled by lmg_spgemm_long_rows (same results, dense accumulator in global
 * scratch: nsets x b_cols doubles and int32 marks, marks zero-initialised by the caller). */
#define LMG_SPGEMM_MAX_ROW_PRODUCTS 8192
int lmg_spgemm_count(int64_t a_rows, const int32_t *d_a_rowptr, const int32_t *d_a_colidx,
                     const int32_t *d_b_rowptr, int32_t *d_row_products, int32_t *d_max_products,
                     void *stream);
int lmg_spgemm_symbolic(int64_t a_rows, const int32_t *d_a_rowptr, const int32_t *d_a_colidx,
                        const int32_t *d_b_rowptr, const int32_t *d_b_colidx,
                        const int32_t *d_row_products, int32_t max_products,
                        int32_t *d_c_rownnz, void *stream);
int lmg_spgemm_numeric(int64_t a_rows, const int32_t *d_a_rowptr, const int32_t *d_a_colidx,
                       const double *d_a_vals, const int32_t *d_b_rowptr,
                       const int32_t *d_b_colidx, const double *d_b_vals,
                       const int32_t *d_row_products, int32_t max_products,
                       const int32_t *d_c_rowptr, int32_t *d_c_colidx, double *d_c_vals,
                       void *stream);
/* Numeric passes on a RECORDED pattern (coefficient changes on a fixed sparsity pattern:
 * the Galerkin rebuild).  lmg_spgemm_numeric_record is lmg_spgemm_numeric that also stores, for
 * every product, its position in the sorted product list of its row (d_dst, uint16, indexed
 * d_prod_ptr[row] + traversal sequence number; d_prod_ptr = exclusive int64 scan of
 * d_row_products with the long rows counted as 0) and the end of every C entry's segment in that
 * list (d_segend[nnz(C)], uint16).  lmg_spgemm_numeric_replay then recomputes d_c_vals without
 * sorting -- same products, same order of additions, bit-identical values -- at 2 bytes of
 * extra traffic per product.  d_c_colidx is not touched by the replay. */
int lmg_spgemm_numeric_record(int64_t a_rows, const int32_t *d_a_rowptr, const int32_t *d_a_colidx,
                              const double *d_a_vals, const int32_t *d_b_rowptr,
                              const int32_t *d_b_colidx, const double *d_b_vals,
                              const int32_t *d_row_products, int32_t max_products,
                              const int32_t *d_c_rowptr, int32_t *d_c_colidx, double *d_c_vals,
                              const int64_t *d_prod_ptr, uint16_t *d_dst, uint16_t *d_segend,
                              void *stream);
int lmg_spgemm_numeric_replay(int64_t a_rows, const int32_t *d_a_rowptr, const int32_t *d_a_colidx,
                              const double *d_a_vals, const int32_t *d_b_rowptr, const double *d_b_vals,
                              const int32_t *d_row_products, int32_t max_products,
                              const int32_t *d_c_rowptr, double *d_c_vals, const int64_t *d_prod_ptr,
                              const uint16_t *d_dst, const uint16_t *d_segend, void *stream);
int lmg_spgemm_long_rows(int numeric, int64_t nlong, const int32_t *d_long_rows,
                         const int32_t *d_a_rowptr, const int32_t *d_a_colidx, const double *d_a_vals,
                         const int32_t *d_b_rowptr, const int32_t *d_b_colidx, const double *d_b_vals,
                         int64_t b_cols, int32_t nsets, double *d_scratch_val, int32_t *d_scratch_mark,
                         int32_t *d_c_rownnz, const int32_t *d_c_rowptr, int32_t *d_c_colidx,
                         double *d_c_vals, void *stream);
/* out[0] = 0, out[i+1] = in[0] + ... + in[i]  (n inputs, n+1 outputs).
 * d_scratch holds lmg_scan_scratch_count(n) int32 values. */
int64_t lmg_scan_scratch_count(int64_t n);
int lmg_exclusive_scan_i32(int64_t n, const int32_t *d_in, int32_t *d_out, int32_t *d_scratch,
                           void *stream);

/* ---- P1 assembly on triangles (the step before the hot path) ----------------------------------
 * Stiffness (optionally element coefficient d_coeff[e]), mass and load vector (constant load
 * f_const) of linear triangles, node-centric and atomic-free; replaces the element loops of
 * assembly/StiffnessMatrix.py:21-36, MassMatrix.py:21-35, LoadVector.py:20-34.
 *   d_px/d_py[n_nodes], d_conn[3*n_elem] (0-based);  node->element adjacency in element order:
 *   d_n2e_ptr[n_nodes+1], d_n2e_elem[], d_n2e_loc[] (local vertex 0..2 of the node in that element);
 *   d_rowptr/d_colidx: the CSR pattern of the mesh graph (node + neighbours), shared by A and M.
 * Any of d_a_vals / d_m_vals / d_rhs may be NULL. */
int lmg_p1_assemble_2d(int64_t n_nodes, const double *d_px, const double *d_py, const int32_t *d_conn,
                       const int32_t *d_n2e_ptr, const int32_t *d_n2e_elem, const int32_t *d_n2e_loc,
                       const double *d_coeff, double f_const, const int32_t *d_rowptr,
                       const int32_t *d_colidx, double *d_a_vals, double *d_m_vals, double *d_rhs,
                       void *stream);

/* ---- 1-D L2-projection coupling operator (the step before the hot path) -------------------------
 * B[i][j] = integral of fine basis i x coarse basis j over the intersections of fine and coarse elements, by
 * the reference's 3-point rule; replaces Intersection.find_intersections1d (Intersection.py:60-76, an
 * O(ne * ne_c) double loop) + CouplingOperator.compute_b_1d (CouplingOperator.py:32-69) and the row
 * scalings of L2Projection.py:74-90.  d_xf / d_xc: strictly increasing node coordinates (nf, nc >= 2).
 * lmg_l2_coupling_count: entries per row; the caller scans them into d_rowptr (lmg_exclusive_scan_i32);
 * lmg_l2_coupling_fill writes sorted CSR rows.  kind 0: B; 1: "pseudo" Q = diag(colsum M_fine)^-1 B;
 * 2: "quasi" Q = B / rowsum(B).  ("L2", Q = M^-1 B, is dense and stays on the host.) */
int lmg_l2_coupling_count(int64_t nf, int64_t nc, const double *d_xf, const double *d_xc, int32_t *d_rownnz,
                          void *stream);
int lmg_l2_coupling_fill(int kind, int64_t nf, int64_t nc, const double *d_xf, const double *d_xc,
                         const int32_t *d_rowptr, int32_t *d_colidx, double *d_vals, void *stream);

/* ---- 2-D L2-projection coupling operator between two P1 triangle meshes (the step before the hot path) ---------
 * B[i][j] = integral of fine basis i x coarse basis j over the intersections of the fine with the coarse elements; the
 * meshes need not be nested or cover the same domain, and elements may have either orientation.  The reference has no
 * 2-D path (L2Projection.compute_transfer_2d is a stub); the rules -- Sutherland-Hodgman clipping, the drop rule
 * area > area_tol * min(|T_e|, |T_c|), the three-point rule of Quadrature.py:87-97 on a fan -- are stated on the host
 * by l2_projection.coupling_operator_2d and in csrc/l2proj2d.hip.  A mesh is d_px / d_py[n] and d_conn[3 * ne]
 * (0-based); f = fine, c = coarse.  Every count must fit int32 (LMG_ERR_ARG otherwise).
 *   limits      candidates per fine element / distinct columns per row the kernels hold (both 64)
 *   d_grid      6 doubles: origin x, y and far corner x, y of the coarse mesh's bounding box, cells per unit length in
 *               x, y (0 for a direction without extent); ncell cells per direction, at most 46340
 *   cell_count  d_count[c] = cells the box of coarse element c overlaps; the caller scans them into d_ptr
 *               (lmg_exclusive_scan_i32), total = their sum
 *   cell_fill   d_keys[d_ptr[c] + k] = cell << 32 | c.  The caller sorts the keys; d_cellptr[cell] is then the first key
 *               of the cell (ncell^2 + 1 entries), d_cellent the low words.
 *   cand_count  d_count[e] = coarse elements whose boxes overlap the box of fine element e (closed boxes); scan into
 *               d_candptr, pairs = their sum, max_count = the largest
 *   cand_fill   d_cand[d_candptr[e] ..]: those elements, ascending, each once.  LMG_ERR_CAPACITY, and nothing launched,
 *               if max_count exceeds the limit.
 *   rows_count  d_rownnz[i] = distinct coarse nodes of row i, limit + 1 for a row with more (one lane per fine node;
 *               d_n2e_*: node -> element adjacency, elements ascending, as for lmg_p1_assemble_2d); scan into
 *               d_rowptr, nnz = their sum, max_row = the largest
 *   rows_fill   sorted CSR rows, each entry accumulated in the order element, candidate, fan triangle, quadrature point,
 *               coarse vertex.  kind 0: B; 1: "pseudo", row i / sum over its elements of |det_e| / 6; 2: "quasi", row i /
 *               its sum.  A row without entries stays empty.  LMG_ERR_CAPACITY, and nothing launched, if max_row
 *               exceeds the limit.  No atomics; two calls give the same bits. */
int lmg_l2p2d_limits(int32_t *max_candidates, int32_t *max_columns);
int lmg_l2p2d_cell_count(int64_t ne_c, const double *d_cpx, const double *d_cpy, const int32_t *d_cconn,
                         const double *d_grid, int32_t ncell, int32_t *d_count, void *stream);
int lmg_l2p2d_cell_fill(int64_t ne_c, const double *d_cpx, const double *d_cpy, const int32_t *d_cconn,
                        const double *d_grid, int32_t ncell, int64_t total, const int32_t *d_ptr, int64_t *d_keys,
                        void *stream);
int lmg_l2p2d_cand_count(int64_t ne_f, const double *d_fpx, const double *d_fpy, const int32_t *d_fconn, int64_t ne_c,
                         const double *d_cpx, const double *d_cpy, const int32_t *d_cconn, const double *d_grid,
                         int32_t ncell, const int32_t *d_cellptr, const int32_t *d_cellent, int32_t *d_count, void *stream);
int lmg_l2p2d_cand_fill(int64_t ne_f, const double *d_fpx, const double *d_fpy, const int32_t *d_fconn, int64_t ne_c,
                        const double *d_cpx, const double *d_cpy, const int32_t *d_cconn, const double *d_grid,
                        int32_t ncell, const int32_t *d_cellptr, const int32_t *d_cellent, int64_t pairs,
                        int32_t max_count, const int32_t *d_candptr, int32_t *d_cand, void *stream);
int lmg_l2p2d_rows_count(int64_t nf, int64_t ne_f, const double *d_fpx, const double *d_fpy, const int32_t *d_fconn,
                         const int32_t *d_n2e_ptr, const int32_t *d_n2e_elem, const int32_t *d_n2e_loc, int64_t nc,
                         int64_t ne_c, const double *d_cpx, const double *d_cpy, const int32_t *d_cconn,
                         const int32_t *d_candptr, const int32_t *d_cand, double area_tol, int32_t *d_rownnz, void *stream);
int lmg_l2p2d_rows_fill(int kind, int64_t nf, int64_t ne_f, const double *d_fpx, const double *d_fpy,
                        const int32_t *d_fconn, const int32_t *d_n2e_ptr, const int32_t *d_n2e_elem,
                        const int32_t *d_n2e_loc, int64_t nc, int64_t ne_c, const double *d_cpx, const double *d_cpy,
                        const int32_t *d_cconn, const int32_t *d_candptr, const int32_t *d_cand, double area_tol, int64_t nnz,
                        int32_t max_row, const int32_t *d_rowptr, int32_t *d_colidx, double *d_vals, void *stream);

/* ---- 2-D learned transfers: what NeuralMG_2D.define_hierarchy does around model.predict ---------------------
 * (Multigrid.py:373-765; the rules: DESIGN.md section 3.)  M: sorted CSR, device.  d_status: ONE 64-bit word the
 * caller sets to UINT64_MAX before a stage and reads after it; a lane that has to refuse writes
 * (order << 8 | rule) with an atomic minimum and leaves, so the word names the first offender: `order` is the row
 * (check), the position among the coarse nodes (count) or the patch (patches, contrib). */
typedef enum {
    LMG_NMG2D_NEGATIVE = 1, /* a negative off-diagonal entry                               */
    LMG_NMG2D_DIAGONAL = 2, /* no positive diagonal entry                                  */
    LMG_NMG2D_VALENCE = 3,  /* a coarse node with 8 or more positive neighbours            */
    LMG_NMG2D_FEW = 4,      /* a coarse node with fewer than 2 neighbours                  */
    LMG_NMG2D_ISOLATED = 5, /* a neighbour whose only positive neighbour is the coarse node */
    LMG_NMG2D_SECOND = 6,   /* more than 6 coarse second neighbours                        */
    LMG_NMG2D_COLUMN = 7    /* an index outside the matrix / a fill index that is not coarse */
} lmg_nmg2d_rule;
/* The domain of the rules, whole matrix, one lane per row: every column inside [0, n), no negative off-diagonal
 * entry, a positive diagonal.  (The reference misaligns `row.nonzero()` and `row[row > 0]` outside it, :634-636.) */
int lmg_nmg2d_check(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                    uint64_t *d_status, void *stream);
/* d_extra[r] = 1 if coarse node d_coarse_nodes[r] has 7 positive neighbours (it gets a second patch), else 0; 8 and
 * more are refused (the first loop of extract_patches, :607-615, whose "works only if neighs are 6 + 1" this is). */
int lmg_nmg2d_count(int64_t nc, const int32_t *d_coarse_nodes, const int32_t *d_rowptr, const int32_t *d_colidx,
                    const double *d_vals, int32_t *d_extra, uint64_t *d_status, void *stream);
/* One lane per patch: d_patches[npatch][43] and d_fill_idx[npatch][31] of coarse node d_patch_node[j], leaving out
 * the d_patch_variant[j]-th smallest neighbour (0 | 1) where the node has 7.  d_rank[n]: position among the coarse
 * nodes, -1 for fine ones.  Replaces extract_patches / single_extraction / direct_neighs / intersecting_rows /
 * create_virtual_nodes (:438-677), which copy and edit one lil row per visit. */
int lmg_nmg2d_patches(int64_t npatch, const int32_t *d_patch_node, const int32_t *d_patch_variant, int64_t n,
                      const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals, const int32_t *d_rank,
                      double *d_patches, int32_t *d_fill_idx, uint64_t *d_status, void *stream);
/* fill_B (:687-732) without the dense n x n_c array, in three steps.  contrib: d_keys[j * 31 + t] = row * nc + col
 * of the entry of B that slot t of patch j is folded into, INT64_MAX for an empty slot.  The caller sorts the keys
 * STABLY (d_slot: the permutation) and finds where the runs of equal keys start (d_start[nentries + 1]).
 * fold: one lane per distinct entry walks its run -- patch order, the order of :691 -- with cur = p if cur == 0 else
 * (cur + p) / 2 (:710-728), p = d_res[slot], and writes the entry as (row, col, val), rows and columns ascending. */
int lmg_nmg2d_contrib(int64_t npatch, int64_t n, int64_t nc, const int32_t *d_fill_idx, const int32_t *d_rank,
                      int64_t *d_keys, uint64_t *d_status, void *stream);
int lmg_nmg2d_fold(int64_t nentries, const int64_t *d_start, const int64_t *d_keys, const int64_t *d_slot,
                   const double *d_res, int64_t nc, int32_t *d_row, int32_t *d_col, double *d_val, void *stream);
/* Q = B with every row divided by its sum, taken in storage order (:758-759 on CSR values; q may be b). */
int lmg_nmg2d_normalize(int64_t n, const int32_t *d_rowptr, const double *d_b_vals, double *d_q_vals, void *stream);
/* d_neighs[nc][6], padded with -1: the coarse positions of fill_idx[7:13] of patch d_last_patch[r] (:704-707). */
int lmg_nmg2d_dneighs(int64_t nc, const int32_t *d_last_patch, const int32_t *d_fill_idx, const int32_t *d_rank,
                      int32_t *d_neighs, void *stream);
/* pre_process (:735-739): entry (i, j) of the coarse mass matrix stays iff j == i or j is in d_neighs[i].  mark
 * counts the kept entries per row; the caller scans them into d_cut_rowptr (lmg_exclusive_scan_i32); fill compacts. */
int lmg_nmg2d_cut_mark(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const int32_t *d_neighs,
                       int32_t *d_rownnz, void *stream);
int lmg_nmg2d_cut_fill(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                       const int32_t *d_neighs, const int32_t *d_cut_rowptr, int32_t *d_cut_colidx,
                       double *d_cut_vals, void *stream);

/* ---- triangle meshes: build, refine, index (the stage before lmg_p1_assemble_2d; csrc/mesh2d.hip) -----------------------
 * What learn_multigrid/mesh/Mesh2D.py does with Python loops (construct :63-93, refine :95-160), the mesh graph that
 * assembly.P1Mesh2D.__init__ states on the host, and the identity rows of thesis_structured_2d.py:407-414.  A mesh is
 * d_px / d_py[n] and d_conn[3 * ne] (0-based).  Sizes: n < 2^31 - 1, 3 * ne < 2^31 - 1, and for a refinement
 * n + edges < 2^31 - 1 (LMG_ERR_ARG otherwise, nothing launched).  d_status: ONE 64-bit word the caller sets to
 * UINT64_MAX before a stage and reads after it, as for lmg_nmg2d_check; the order is the element (check) or the row
 * (identity rows), so the lowest offender is named.  A slot s = 3 e + k is the directed edge conn[e][k] ->
 * conn[e][(k + 1) % 3].
 *   limits      distinct columns per pattern row the kernels hold (64)
 *   construct   h_el x v_el squares on the unit square: nodes row-major, h fastest, coordinate i * (1.0 / N) and exactly
 *               1.0 for i = N (np.linspace); square k gives (k, k+1, k+W+1) then (k, k+W+1, k+W), W = h_el + 1.
 *               d_px / d_py[(h_el + 1)(v_el + 1)], d_conn[6 h_el v_el]
 *   check       one lane per element: every index inside [0, n), no repeated vertex
 *   edge_keys   d_keys[s] = min(left, right) << 32 | max(left, right).  The caller sorts the keys STABLY with their
 *               slots (d_slot: the permutation); a run of equal keys is one undirected edge, its head its smallest slot.
 *   edge_runs   d_head[s] = the head slot of the run of s, d_is_head[s] = 1 for a head, else 0 (the caller scans them
 *               into d_rank with lmg_exclusive_scan_i32: edges = their sum).  d_mask (bytes, zeroed by the caller, may
 *               be null): 1 on both ends of every run of length 1 -- the boundary nodes.  Runs longer than 2 are allowed.
 *   refine      nodes 0 .. n-1 are copied; the midpoint of a run is node n + d_rank[head], written by the head slot's
 *               lane as r * p[left] + (1 - r) * p[right], r = 0.5 or d_ratio[node - n]; element e becomes
 *               [t0 v1 t1] [t1 v2 t2] [t0 t1 t2] [v0 t0 t2] at 4 e .. 4 e + 3, t_k the midpoint of slot k.  Outputs
 *               d_px_out / d_py_out[n + edges], d_conn_out[12 ne] must not be the inputs.
 *   n2e_fill    d_order: the permutation of a STABLE sort of d_conn by node; d_elem = order / 3, d_loc = order % 3 (the
 *               adjacency of lmg_p1_assemble_2d, elements ascending per node; d_n2e_ptr is the caller's search)
 *   rows_count  d_rownnz[i] = distinct vertices of the elements of node i (0 for a node in no element), limit + 1 for a
 *               row with more; one lane per node, the set sorted in LDS; scan into d_rowptr, nnz = their sum,
 *               max_row = the largest
 *   rows_fill   d_colidx: the sorted pattern rows.  LMG_ERR_CAPACITY, and nothing launched, if max_row exceeds the limit.
 *   lmg_csr_identity_rows   for every row i with d_mask[i] != 0: 1.0 on the diagonal, 0.0 on the row's other stored
 *               entries, in place (columns untouched), and d_rhs[i] = 0, or d_value[i] where d_value is given (d_rhs may
 *               be null).  A masked row without a stored diagonal is refused, and then no row is changed.
 * No floating-point atomics; two calls give the same bits in every output array. */
typedef enum {
    LMG_MESH2D_INDEX = 1,    /* a vertex index outside [0, n)            */
    LMG_MESH2D_REPEATED = 2, /* an element with a repeated vertex        */
    LMG_MESH2D_DIAGONAL = 3  /* a masked row without a stored diagonal   */
} lmg_mesh2d_rule;
int lmg_mesh2d_limits(int32_t *max_columns);
int lmg_mesh2d_construct(int64_t h_el, int64_t v_el, double *d_px, double *d_py, int32_t *d_conn, void *stream);
int lmg_mesh2d_check(int64_t n, int64_t ne, const int32_t *d_conn, uint64_t *d_status, void *stream);
int lmg_mesh2d_edge_keys(int64_t ne, const int32_t *d_conn, int64_t *d_keys, void *stream);
int lmg_mesh2d_edge_runs(int64_t n, int64_t ne, const int64_t *d_keys, const int64_t *d_slot, int32_t *d_head,
                         int32_t *d_is_head, uint8_t *d_mask, void *stream);
int lmg_mesh2d_refine(int64_t n, int64_t ne, int64_t edges, const double *d_px, const double *d_py, const int32_t *d_conn,
                      const int32_t *d_head, const int32_t *d_rank, const double *d_ratio, double *d_px_out,
                      double *d_py_out, int32_t *d_conn_out, void *stream);
int lmg_mesh2d_n2e_fill(int64_t ne, const int64_t *d_order, int32_t *d_elem, int32_t *d_loc, void *stream);
int lmg_mesh2d_rows_count(int64_t n, int64_t ne, const int32_t *d_conn, const int32_t *d_n2e_ptr,
                          const int32_t *d_n2e_elem, int32_t *d_rownnz, void *stream);
int lmg_mesh2d_rows_fill(int64_t n, int64_t ne, const int32_t *d_conn, const int32_t *d_n2e_ptr,
                         const int32_t *d_n2e_elem, int64_t nnz, int32_t max_row, const int32_t *d_rowptr,
                         int32_t *d_colidx, void *stream);
int lmg_csr_identity_rows(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, double *d_vals,
                          const uint8_t *d_mask, const double *d_value, double *d_rhs, uint64_t *d_status, void *stream);

/* ---- classical AMG setup: from A to P with nothing else given (csrc/amg.hip; the stages: amg.py) ------------------------------
 * What pyamg.ruge_stuben_solver does on the host in the reference's experiment scripts (test_pyAMG.py), with the PMIS split in
 * place of Ruge-Stueben's sequential passes.  The rules: DESIGN.md section 3, "Classical AMG setup".  A: sorted, duplicate-free
 * CSR on the device, n < 2^31 - 257.  One lane per row, no atomics, no scratch; two calls give the same integers and bits.
 * Every pointer an entry point names must be non-null (LMG_ERR_ARG, nothing launched) -- a matrix without entries hands in
 * any valid address for its entry arrays --, theta and trunc lie in [0, 1], omega is finite.  n == 0: LMG_OK.
 *   strength    m_ij = -sign(a_ii) a_ij, j != i; j is strong iff m_ij > 0 and m_ij >= theta * max_k m_ik.  count: entries per
 *               row of S (0 for a row with no or a zero diagonal); the caller scans them (lmg_exclusive_scan_i32); fill: the
 *               strong columns in A's order.
 *   pmis_keys   d_count[i] = row length of S^T (how many rows i is strong for), d_state[i] = LMG_AMG_FINE0 for an empty row of
 *               S, else LMG_AMG_UNDECIDED, d_is_coarse[i] = 0.
 *   pmis_select d_flag[i] = 1 iff i is undecided and (count, hash, index) of i exceeds that of every undecided neighbour in
 *               S_i and S^T_i, compared lexicographically; hash: x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15,
 *               x *= 0x846ca68b, x ^= x >> 16 on uint32.
 *   pmis_update a flagged node becomes LMG_AMG_COARSE, another undecided node with a flagged j in S_i LMG_AMG_FINE;
 *               d_is_coarse[i] = 1 | 0 for every i; d_block_undecided[b], b < lmg_amg_pmis_blocks(n): the undecided nodes left
 *               among rows 256 b .. 256 b + 255.  The host sums them and launches the next round while the sum is positive.
 *   interp      direct interpolation into P (n x n_c).  d_rank[i]: the number of coarse nodes below i.  A coarse row: 1.0 at
 *               rank[i].  A fine row i with C_i = S_i and coarse: d = a_ii + (sum of the a_ik, k != i, of a_ii's sign),
 *               alpha = (sum of the a_ik of the other sign) / (sum over C_i), P_ij = -(alpha a_ij) / d at column rank[j],
 *               sums in storage order.  FINE0 rows and fine rows with an empty C_i stay empty.  d zero or not finite: refused
 *               through d_status (ONE 64-bit word set to UINT64_MAX by the caller, row << 8 | LMG_AMG_PIVOT by an atomic
 *               minimum, as for lmg_nmg2d_check).  count: entries per row; fill: after the caller's scan.
 *   smooth      one Jacobi step on P with truncation, AP = A P from lmg_spgemm_*: a fine row takes the pattern of AP_i and
 *               v_c = P_ic - (omega AP_ic) / a_ii (P_ic = 0 where absent); entries with |v_c| < trunc * max_c |v_c| leave, the
 *               others are multiplied by (sum of all v_c) / (sum of the kept) unless that sum is 0.  Coarse rows stay 1.0 at
 *               rank[i], FINE0 rows empty.  count: entries per row; fill: after the caller's scan. */
typedef enum {
    LMG_AMG_UNDECIDED = 0,
    LMG_AMG_COARSE = 1,
    LMG_AMG_FINE = 2,
    LMG_AMG_FINE0 = 3 /* a row with no strong entry: fine at once, never coarse, empty row of P */
} lmg_amg_state;
typedef enum {
    LMG_AMG_PIVOT = 1,     /* d_i of a fine row is zero or not finite */
    LMG_AMG_CANDIDATE = 2, /* lmg_sa_norms: the candidate's sum of squares over an aggregate is zero or not finite */
    LMG_AMG_MEMBERS = 3    /* lmg_sa_norms: the member list of an aggregate does not ascend (order: the aggregate) */
} lmg_amg_rule;
int lmg_amg_strength_count(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals, double theta,
                           int32_t *d_rownnz, void *stream);
int lmg_amg_strength_fill(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals, double theta,
                          const int32_t *d_s_rowptr, int32_t *d_s_colidx, void *stream);
int lmg_amg_pmis_keys(int64_t n, const int32_t *d_s_rowptr, const int32_t *d_st_rowptr, int32_t *d_count, int32_t *d_state,
                      int32_t *d_is_coarse, void *stream);
int lmg_amg_pmis_select(int64_t n, const int32_t *d_s_rowptr, const int32_t *d_s_colidx, const int32_t *d_st_rowptr,
                        const int32_t *d_st_colidx, const int32_t *d_count, const int32_t *d_state, int32_t *d_flag,
                        void *stream);
int64_t lmg_amg_pmis_blocks(int64_t n);
int lmg_amg_pmis_update(int64_t n, const int32_t *d_s_rowptr, const int32_t *d_s_colidx, const int32_t *d_flag,
                        int32_t *d_state, int32_t *d_is_coarse, int32_t *d_block_undecided, void *stream);
int lmg_amg_interp_count(int64_t n, const int32_t *d_s_rowptr, const int32_t *d_s_colidx, const int32_t *d_state,
                         int32_t *d_rownnz, void *stream);
int lmg_amg_interp_fill(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                        const int32_t *d_s_rowptr, const int32_t *d_s_colidx, const int32_t *d_state, const int32_t *d_rank,
                        const int32_t *d_p_rowptr, int32_t *d_p_colidx, double *d_p_vals, uint64_t *d_status, void *stream);
int lmg_amg_smooth_count(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                         const int32_t *d_p_rowptr, const int32_t *d_p_colidx, const double *d_p_vals,
                         const int32_t *d_ap_rowptr, const int32_t *d_ap_colidx, const double *d_ap_vals,
                         const int32_t *d_state, const int32_t *d_rank, double omega, double trunc, int32_t *d_rownnz,
                         void *stream);
int lmg_amg_smooth_fill(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                        const int32_t *d_p_rowptr, const int32_t *d_p_colidx, const double *d_p_vals,
                        const int32_t *d_ap_rowptr, const int32_t *d_ap_colidx, const double *d_ap_vals,
                        const int32_t *d_state, const int32_t *d_rank, double omega, double trunc,
                        const int32_t *d_q_rowptr, int32_t *d_q_colidx, double *d_q_vals, void *stream);

/* ---- smoothed-aggregation setup: from A and one candidate B to the tentative prolongator (csrc/sa.hip; the stages:
 * aggregation.py).  What pyamg.smoothed_aggregation_solver does on the host, with MIS-2 aggregates in place of pyamg's sequential
 * standard aggregation.  The rules: DESIGN.md section 3, "Smoothed aggregation setup".  A: sorted, duplicate-free CSR on the
 * device, n < 2^31 - 257.  One lane per row (lmg_sa_norms: per aggregate), no atomics but the refusals, no scratch; every kernel
 * reads what an earlier launch wrote and writes its own lane's entries, so two calls give the same integers and bits.  Every
 * pointer an entry point names must be non-null (LMG_ERR_ARG, nothing launched), theta lies in [0, 1].  n == 0: LMG_OK.
 *   diagonal    d_diag[i] = the stored a_ii, 0.0 where there is none.
 *   strength    j is strong in row i iff j != i, a_ij != 0, a_ii != 0, a_jj != 0 and a_ij a_ij >= (theta theta) |a_ii a_jj|,
 *               every product rounded on its own.  count: entries per row of S; fill: the strong columns in A's order, after the
 *               caller's scan.  A node whose row of S is empty is isolated.
 *   graph       G_i = the ascending merge of S_i and S^T_i (lmg_csr_transpose_*) without i and without isolated nodes; empty
 *               for an isolated i.  count / fill as above.
 *   mis2_init   d_state[i] = LMG_SA_ISOLATED for an empty row of S, else LMG_SA_UNDECIDED; d_is_root[i] = 0.
 *   mis2_t1     d_t1[i] = the undecided node of the largest key in N[i] = {i} u G_i, or -1.  Key: (row length of G, hash, index),
 *               compared lexicographically, the hash of lmg_amg_pmis_select.
 *   mis2_t2     d_flag[i] = 1 iff i is undecided and the node of the largest key among d_t1[j], j in N[i], is i.
 *   mis2_c1     d_c1[i] = 1 iff some node of N[i] is flagged.
 *   mis2_update a flagged node becomes LMG_SA_ROOT, another undecided node with some d_c1[j], j in N[i], LMG_SA_COVERED;
 *               d_is_root[i] = 1 | 0 for every i; d_block_undecided[b], b < lmg_sa_blocks(n): the undecided nodes left among
 *               rows 256 b .. 256 b + 255.  The host sums them and launches the next round while the sum is positive.
 *   assign1     d_rank[i]: the number of roots below i.  A root: d_a1[i] = d_rank[i]; a covered node with roots in G_i: the
 *               rank of the one of the largest key; every other node -1.
 *   assign2     d_a2[i] = d_a1[i] where that is >= 0 or i is isolated, else d_a1[j] of the largest-key j in G_i with
 *               d_a1[j] >= 0 (-1 without one).  d_a1 != d_a2.
 *   tentative   count: 1 for a row with 0 <= d_agg[i] < n_agg, else 0.  pattern, after the caller's scan: column d_agg[i], value
 *               d_cand[i] -- the transpose of this matrix lists the members of every aggregate with their candidate values.
 *               fill: d_t_vals = d_cand[i] / d_coarse_cand[d_agg[i]] on the same pattern.
 *   norms       one lane per aggregate j on that transpose: s = the sum of the squared values in storage order,
 *               d_coarse_cand[j] = sqrt(s).  s zero or not finite: refused through d_status (as lmg_amg_interp_fill) with the
 *               first member row and LMG_AMG_CANDIDATE; a member list that does not ascend: the aggregate and LMG_AMG_MEMBERS.
 *   row_states  d_state[i] = LMG_AMG_FINE for a row of T with an entry, else LMG_AMG_FINE0: what lmg_amg_smooth_* reads for
 *               the Jacobi step on T (omega = omega_sa / rho, trunc = 0). */
typedef enum {
    LMG_SA_UNDECIDED = 0,
    LMG_SA_ROOT = 1,
    LMG_SA_COVERED = 2, /* within two edges of a root */
    LMG_SA_ISOLATED = 3 /* an empty row of S: no aggregate, never a neighbour, empty row of P */
} lmg_sa_state;
int lmg_sa_diagonal(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals, double *d_diag,
                    void *stream);
int lmg_sa_strength_count(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                          const double *d_diag, double theta, int32_t *d_rownnz, void *stream);
int lmg_sa_strength_fill(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                         const double *d_diag, double theta, const int32_t *d_s_rowptr, int32_t *d_s_colidx, void *stream);
int lmg_sa_graph_count(int64_t n, const int32_t *d_s_rowptr, const int32_t *d_s_colidx, const int32_t *d_st_rowptr,
                       const int32_t *d_st_colidx, int32_t *d_rownnz, void *stream);
int lmg_sa_graph_fill(int64_t n, const int32_t *d_s_rowptr, const int32_t *d_s_colidx, const int32_t *d_st_rowptr,
                      const int32_t *d_st_colidx, const int32_t *d_g_rowptr, int32_t *d_g_colidx, void *stream);
int lmg_sa_mis2_init(int64_t n, const int32_t *d_s_rowptr, int32_t *d_state, int32_t *d_is_root, void *stream);
int lmg_sa_mis2_t1(int64_t n, const int32_t *d_g_rowptr, const int32_t *d_g_colidx, const int32_t *d_state, int32_t *d_t1,
                   void *stream);
int lmg_sa_mis2_t2(int64_t n, const int32_t *d_g_rowptr, const int32_t *d_g_colidx, const int32_t *d_state,
                   const int32_t *d_t1, int32_t *d_flag, void *stream);
int lmg_sa_mis2_c1(int64_t n, const int32_t *d_g_rowptr, const int32_t *d_g_colidx, const int32_t *d_state,
                   const int32_t *d_flag, int32_t *d_c1, void *stream);
int64_t lmg_sa_blocks(int64_t n);
int lmg_sa_mis2_update(int64_t n, const int32_t *d_g_rowptr, const int32_t *d_g_colidx, const int32_t *d_flag,
                       const int32_t *d_c1, int32_t *d_state, int32_t *d_is_root, int32_t *d_block_undecided, void *stream);
int lmg_sa_assign1(int64_t n, const int32_t *d_g_rowptr, const int32_t *d_g_colidx, const int32_t *d_state,
                   const int32_t *d_rank, int32_t *d_a1, void *stream);
int lmg_sa_assign2(int64_t n, const int32_t *d_g_rowptr, const int32_t *d_g_colidx, const int32_t *d_state,
                   const int32_t *d_a1, int32_t *d_a2, void *stream);
int lmg_sa_tentative_count(int64_t n, int64_t n_agg, const int32_t *d_agg, int32_t *d_rownnz, void *stream);
int lmg_sa_tentative_pattern(int64_t n, int64_t n_agg, const int32_t *d_agg, const double *d_cand, const int32_t *d_t_rowptr,
                             int32_t *d_t_colidx, double *d_t_vals, void *stream);
int lmg_sa_norms(int64_t n_agg, const int32_t *d_m_rowptr, const int32_t *d_m_colidx, const double *d_m_vals,
                 double *d_coarse_cand, uint64_t *d_status, void *stream);
int lmg_sa_tentative_fill(int64_t n, int64_t n_agg, const int32_t *d_agg, const double *d_cand, const double *d_coarse_cand,
                          const int32_t *d_t_rowptr, double *d_t_vals, void *stream);
int lmg_sa_row_states(int64_t n, const int32_t *d_t_rowptr, int32_t *d_state, void *stream);

/* ---- smoothed aggregation for systems: node blocks of bs unknowns and k <= LMG_NSP_MAX_CANDIDATES candidates (csrc/nsp.hip; the
 * stages: aggregation.py).  What pyamg.smoothed_aggregation_solver(A, B) does with a BSR matrix and B of shape (n, k).  The rules:
 * DESIGN.md section 3, "Smoothed aggregation for systems".  A: sorted, duplicate-free CSR on the device, n = bs n_nodes unknowns,
 * n < 2^31 - 257 and k n_agg < 2^31 - 257; the unknowns bs I .. bs I + bs - 1 belong to node I.  One lane per row (condense: per
 * node row; gram_chol, tri_product: per aggregate), no atomics but the refusals, no scratch; every kernel reads what an earlier
 * launch wrote and writes its own lane's entries, so two calls give the same integers and bits.  Every product and sum rounds on
 * its own, every sum starts from 0.0.  Every pointer an entry point names must be non-null (LMG_ERR_ARG, nothing launched), bs >= 1,
 * 1 <= k <= LMG_NSP_MAX_CANDIDATES, 0 <= n_agg <= n_nodes, rank_tol finite and positive.  Nothing to do (n_nodes == 0, n == 0,
 * n_agg == 0): LMG_OK.
 *   condense    C (n_nodes x n_nodes): an entry (I, J) iff some stored a_ij lies in that block, explicit zeros included; columns
 *               ascend; c_IJ = sqrt(sum a_ij a_ij) over the rows of the block ascending and in storage order within a row.
 *               count: entries per node row; fill: after the caller's scan.  lmg_sa_* run on C unchanged.
 *   gram_chol   d_m_rowptr / d_m_colidx: row j lists the member NODES of aggregate j in ascending order (the transpose of
 *               lmg_sa_tentative_pattern on the node aggregates).  d_x: n x k row-major.  g_pq = sum x_ip x_iq (p <= q) over the
 *               member rows, the nodes ascending and the unknowns within a node ascending.  For c = 0 .. k-1, r = 0 .. c:
 *               s = g_rc - R_0r R_0c - ... - R_(r-1)r R_(r-1)c in that order; r < c: R_rc = s / R_rr; r = c: R_cc = sqrt(s), and
 *               unless s is finite and s > rank_tol g_cc the aggregate is refused through d_status (as lmg_sa_norms) with
 *               bs * (its smallest member node) and LMG_AMG_CANDIDATE; a member list that does not ascend: the aggregate and
 *               LMG_AMG_MEMBERS.  d_r: n_agg x k x k row-major, zeros below the diagonal.
 *   apply       for every unknown i of a node with 0 <= d_agg[node] < n_agg: y_0 = x_0 / R_00,
 *               y_c = (x_c - y_0 R_0c - ... - y_(c-1) R_(c-1)c) / R_cc with the R of that aggregate; other rows of d_y are left
 *               as they are.  d_agg: per NODE.  d_x != d_y.
 *   tri_product d_coarse_cand (k n_agg x k row-major): block j = R2_j R1_j, entry (r, c) = sum over q = r .. c of
 *               R2_rq R1_qc, q ascending; zeros below the diagonal.
 *   tentative   count: k for a row of an aggregated node, else 0.  fill, after the caller's scan: the columns k agg + c,
 *               c = 0 .. k-1, with the values y R2^-1 (as apply) of row i of d_y -- the second round written straight into T. */
#define LMG_NSP_MAX_CANDIDATES 6
int lmg_nsp_condense_count(int64_t n_nodes, int32_t bs, const int32_t *d_rowptr, const int32_t *d_colidx, int32_t *d_rownnz,
                           void *stream);
int lmg_nsp_condense_fill(int64_t n_nodes, int32_t bs, const int32_t *d_rowptr, const int32_t *d_colidx, const double *d_vals,
                          const int32_t *d_c_rowptr, int32_t *d_c_colidx, double *d_c_vals, void *stream);
int lmg_nsp_gram_chol(int64_t n_agg, int64_t n_nodes, int32_t bs, int32_t k, const int32_t *d_m_rowptr,
                      const int32_t *d_m_colidx, const double *d_x, double rank_tol, double *d_r, uint64_t *d_status,
                      void *stream);
int lmg_nsp_apply(int64_t n, int64_t n_agg, int32_t bs, int32_t k, const int32_t *d_agg, const double *d_x, const double *d_r,
                  double *d_y, void *stream);
int lmg_nsp_tri_product(int64_t n_agg, int32_t k, const double *d_r2, const double *d_r1, double *d_coarse_cand, void *stream);
int lmg_nsp_tentative_count(int64_t n, int64_t n_agg, int32_t bs, int32_t k, const int32_t *d_agg, int32_t *d_rownnz,
                            void *stream);
int lmg_nsp_tentative_fill(int64_t n, int64_t n_agg, int32_t bs, int32_t k, const int32_t *d_agg, const double *d_y,
                           const double *d_r2, const int32_t *d_t_rowptr, int32_t *d_t_colidx, double *d_t_vals, void *stream);

/* ---- multicolour Gauss-Seidel with its setup on the device (csrc/color.hip; the stages: ops.build_gs_schedule_device) ---------
 * The rules: DESIGN.md section 3, "Multicolour Gauss-Seidel on the device".  A: CSR on the device, n < 2^31 - 257; T: its
 * transpose (lmg_csr_transpose_*); G: the pattern of A and T without the diagonal, stored zeros included.  One lane per row (the
 * twin and the sweep: one wave per slice of 64 scheduled rows), no atomics but the refusal, no scratch; every kernel reads what
 * an earlier launch wrote and writes its own lane's entries, so two calls give the same integers and bits.  Every pointer an
 * entry point names must be non-null (LMG_ERR_ARG, nothing launched) -- a matrix without entries hands in any valid address for
 * its entry arrays.  n == 0 (nslices == 0, padded == 0, ncolors == 0, sweeps == 0): LMG_OK.
 *   select      d_color[i] < 0: uncoloured (the caller starts with -1 everywhere).  d_flag[i] = 1 iff i is uncoloured and
 *               (hash, index) of i exceeds that of every uncoloured neighbour in G, compared lexicographically; the hash of
 *               lmg_amg_pmis_select.  A node without neighbours is flagged in the first round.
 *   assign      a flagged node takes the smallest colour c >= 0 that no coloured neighbour has.  One that would need colour
 *               LMG_COLOR_MAX is refused through d_status (ONE 64-bit word set to UINT64_MAX by the caller, the node's number
 *               by an atomic minimum) and stays uncoloured.  d_block_uncolored[b], b < lmg_color_blocks(n): the uncoloured nodes
 *               left among rows 256 b .. 256 b + 255.  The host sums them and launches the next round while the sum is positive;
 *               a round that colours nothing means a refusal.
 *   twin_count  the schedule: d_rows ordered by (colour, row), d_color_ptr[c] its first position of colour c (ncolors + 1
 *               entries, every colour with a row).  Colour c owns the slices d_color_slice[c] .. d_color_slice[c + 1] - 1,
 *               (rows of c + 63) / 64 of them.  d_twin_row[64 s + t] = the row of lane t of slice s, -1 beyond the colour's
 *               last row; d_twin_len: its entries (0 for -1); d_slice_len[s]: the longest of the slice.
 *   twin_fill   d_slice_base[s] = 64 * (the sum of d_slice_len below s).  Entry j of the row at lane t of slice s goes to
 *               position d_slice_base[s] + 64 j + t of d_col, d_val and d_src (its index in d_vals); positions no entry goes to
 *               keep what the caller put there (d_src: -1).
 *   twin_refill d_val[p] = d_vals[d_src[p]] for the padded positions with d_src[p] >= 0: new values on the same pattern.
 *   sweep       `sweeps` sweeps in place on d_x over the colours 0 .. ncolors - 1 (backward = 1: ncolors - 1 .. 0), one launch
 *               per colour; h_color_slice: the HOST copy of d_color_slice.  Per row the update of lmg_csr_gs_schedule: rsum over
 *               the entries off the diagonal in storage order with separately rounded products, diag the last stored entry
 *               on it, x[row] = (b[row] - rsum) / diag; a row without a diagonal or with diag == 0 is left as it is.  The same
 *               bits as lmg_csr_gs_schedule on d_rows / d_color_ptr (backward: on the reversed row list).  max_len: the
 *               largest d_slice_len, padded: 64 * their sum (they pick the unroll factor and the nontemporal loads of
 *               lmg_sell_sweep).  No LDS, no barrier, capture-safe. */
#define LMG_COLOR_MAX 64 /* colours 0 .. 63 */
int lmg_color_select(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const int32_t *d_t_rowptr,
                     const int32_t *d_t_colidx, const int32_t *d_color, int32_t *d_flag, void *stream);
int64_t lmg_color_blocks(int64_t n);
int lmg_color_assign(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, const int32_t *d_t_rowptr,
                     const int32_t *d_t_colidx, const int32_t *d_flag, int32_t *d_color, int32_t *d_block_uncolored,
                     uint64_t *d_status, void *stream);
int lmg_color_twin_count(int64_t nslices, int32_t ncolors, const int32_t *d_color_ptr, const int32_t *d_color_slice,
                         const int32_t *d_rows, const int32_t *d_rowptr, int32_t *d_twin_row, int32_t *d_twin_len,
                         int32_t *d_slice_len, void *stream);
int lmg_color_twin_fill(int64_t nslices, const int32_t *d_twin_row, const int32_t *d_rowptr, const int32_t *d_colidx,
                        const double *d_vals, const int64_t *d_slice_base, int32_t *d_col, double *d_val, int32_t *d_src,
                        void *stream);
int lmg_color_twin_refill(int64_t padded, const int32_t *d_src, const double *d_vals, double *d_val, void *stream);
int lmg_color_sweep(int32_t ncolors, const int32_t *h_color_slice, const int64_t *d_slice_base, const int32_t *d_slice_len,
                    const int32_t *d_twin_row, const int32_t *d_twin_len, const int32_t *d_col, const double *d_val,
                    int32_t max_len, int64_t padded, double *d_x, const double *d_b, int sweeps, int backward, void *stream);

/* ---- hipGraph capture of a launch sequence (one V-cycle) -----------------------------
 * begin/end bracket launches issued on `stream`; end returns an opaque executable graph. */
int lmg_graph_begin(void *stream);
int lmg_graph_end(void *stream, void **graph_exec_out);
int lmg_graph_launch(void *graph_exec, void *stream);
int lmg_graph_destroy(void *graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* LMG_H */
