// Smoothed-aggregation setup on the device (aggregation.py): from a matrix A and one near-nullspace candidate B to the tentative
// prolongator T, with nothing else given.  What pyamg.smoothed_aggregation_solver does on the host, with aggregates that are
// found in parallel (MIS-2 roots in place of pyamg's sequential standard aggregation).  The rules: DESIGN.md section 3,
// "Smoothed aggregation setup"; the plain-Python restatement the kernels are compared with bit for bit: tests/sa_ref.py.
//   - diagonal:       diag[i] = the stored a_ii, 0.0 where there is none;
//   - strength count / fill:  j is strong in row i iff j != i, a_ij != 0, a_ii != 0, a_jj != 0 and
//             a_ij a_ij >= (theta theta) |a_ii a_jj|, every product rounded on its own, no square root.  S keeps the strong
//             columns in A's order.  An empty row of S is an ISOLATED node: no aggregate, an empty row of P;
//   - graph count / fill:  G_i = the merge of the sorted rows S_i and S^T_i without the isolated nodes; empty for an isolated i.
//             Every later kernel walks G only;
//   - mis2 init:      ISOLATED for an empty row of S, else UNDECIDED;
//   - mis2 t1:        t1[i] = the undecided node of the largest key (deg_G, hash(i), i) in N[i] = {i} u G_i, or -1;
//   - mis2 t2:        t2 = the node of the largest key among the t1[j], j in N[i]; an undecided i with t2 == i is flagged;
//   - mis2 c1:        c1[i] = some flag in N[i];
//   - mis2 update:    a flagged node becomes a ROOT, another undecided node with some c1[j], j in N[i], COVERED (it is within two
//             edges of a root); the undecided nodes left are counted per workgroup (the host reads their sum, one count per
//             round, and launches the next round);
//   - assign 1 / 2:   a root takes its rank; a covered node next to roots joins the one of the largest key (a1); a node still
//             without an aggregate takes a1[j] of the largest-key j in G_i that has one (reads a1, writes a2);
//   - tentative count / pattern:  one entry per aggregated row, column agg[i], value B_i -- the n x n_agg pattern whose
//             transpose (lmg_csr_transpose_*) lists the members of every aggregate in ascending order, with their B;
//   - norms:          one lane per aggregate: s_j = the sum of B_i B_i over its members, i ascending; Bc_j = sqrt(s_j);
//   - tentative fill: T_ij = B_i / Bc_j.
// Every kernel reads arrays an earlier launch wrote and writes its own lane's entries, so the result does not depend on the
// launch geometry.  No atomics but the refusals, which report (row << 8 | rule) with an atomic minimum on one 64-bit status word
// like amg.hip.  Nothing waits for another workgroup.  No local arrays: no scratch.
#include "lmg_common.hpp"

#include <climits>

namespace {

constexpr int kB = 256;
enum { UNDECIDED = LMG_SA_UNDECIDED, ROOT = LMG_SA_ROOT, COVERED = LMG_SA_COVERED, ISOLATED = LMG_SA_ISOLATED };

__device__ __forceinline__ void refuse(unsigned long long *status, long long order, int rule)
{
    atomicMin(status, ((unsigned long long)order << 8) | (unsigned long long)rule);
}

__device__ __forceinline__ bool in_range(int n, int j) { return (unsigned)j < (unsigned)n; }

// ---- strength ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kB) diagonal_kernel(int n, const int *Ap, const int *Aj, const double *Av, double *diag)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    double d = 0.0;
    for (int k = Ap[i]; k < Ap[i + 1]; ++k)
        if (Aj[k] == i) d = Av[k];
    diag[i] = d;
}

__device__ __forceinline__ bool is_strong(int n, int i, double di, int j, double v, const double *diag, double tt)
{
    if (j == i || !in_range(n, j) || !(v != 0.0) || !(di != 0.0)) return false;
    const double dj = diag[j];
    if (!(dj != 0.0)) return false;
    return v * v >= tt * fabs(di * dj);
}

__global__ void __launch_bounds__(kB) strength_count_kernel(int n, const int *Ap, const int *Aj, const double *Av,
                                                            const double *diag, double theta, int *rownnz)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const double di = diag[i], tt = theta * theta;
    int c = 0;
    for (int k = Ap[i]; k < Ap[i + 1]; ++k) c += is_strong(n, i, di, Aj[k], Av[k], diag, tt) ? 1 : 0;
    rownnz[i] = c;
}

__global__ void __launch_bounds__(kB) strength_fill_kernel(int n, const int *Ap, const int *Aj, const double *Av,
                                                           const double *diag, double theta, const int *Sp, int *Sj)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const double di = diag[i], tt = theta * theta;
    int at = Sp[i];
    const int end = Sp[i + 1];
    for (int k = Ap[i]; k < Ap[i + 1]; ++k)
        if (is_strong(n, i, di, Aj[k], Av[k], diag, tt) && at < end) Sj[at++] = Aj[k];
}

// ---- the aggregation graph ----------------------------------------------------------------------------------------------
// The merge of the ascending rows S_i and S^T_i, entry by entry: f(j) for every distinct j != i whose row of S has entries.
template <typename F>
__device__ __forceinline__ void graph_row(int n, int i, const int *Sp, const int *Sj, const int *STp, const int *STj, F &&f)
{
    int a = Sp[i], b = STp[i];
    const int ae = Sp[i + 1], be = STp[i + 1];
    if (a >= ae) return;                                   // an isolated node has no neighbours
    while (a < ae || b < be) {
        const int ja = a < ae ? Sj[a] : INT_MAX, jb = b < be ? STj[b] : INT_MAX;
        const int j = ja < jb ? ja : jb;
        if (ja == j) ++a;
        if (jb == j) ++b;
        if (j != i && in_range(n, j) && Sp[j + 1] > Sp[j]) f(j);
    }
}

__global__ void __launch_bounds__(kB) graph_count_kernel(int n, const int *Sp, const int *Sj, const int *STp, const int *STj,
                                                         int *rownnz)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    int c = 0;
    graph_row(n, i, Sp, Sj, STp, STj, [&](int) { ++c; });
    rownnz[i] = c;
}

__global__ void __launch_bounds__(kB) graph_fill_kernel(int n, const int *Sp, const int *Sj, const int *STp, const int *STj,
                                                        const int *Gp, int *Gj)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    int at = Gp[i];
    const int end = Gp[i + 1];
    graph_row(n, i, Sp, Sj, STp, STj, [&](int j) {
        if (at < end) Gj[at++] = j;
    });
}

// ---- MIS-2 roots --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned hash32(unsigned x)
{
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// whether the key (deg_G, hash, index) of node a exceeds that of node b; any node exceeds b = -1
__device__ __forceinline__ bool exceeds(int a, int b, const int *Gp)
{
    if (b < 0) return true;
    const int da = Gp[a + 1] - Gp[a], db = Gp[b + 1] - Gp[b];
    if (da != db) return da > db;
    const unsigned ha = hash32((unsigned)a), hb = hash32((unsigned)b);
    if (ha != hb) return ha > hb;
    return a > b;
}

__global__ void __launch_bounds__(kB) mis2_init_kernel(int n, const int *Sp, int *state, int *is_root)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    state[i] = Sp[i + 1] > Sp[i] ? UNDECIDED : ISOLATED;
    is_root[i] = 0;
}

__global__ void __launch_bounds__(kB) mis2_t1_kernel(int n, const int *Gp, const int *Gj, const int *state, int *t1)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const int st = state[i];
    int best = st == UNDECIDED ? i : -1;
    if (st != ISOLATED)
        for (int k = Gp[i]; k < Gp[i + 1]; ++k) {
            const int j = Gj[k];
            if (in_range(n, j) && state[j] == UNDECIDED && exceeds(j, best, Gp)) best = j;
        }
    t1[i] = best;
}

__global__ void __launch_bounds__(kB) mis2_t2_kernel(int n, const int *Gp, const int *Gj, const int *state, const int *t1,
                                                     int *flag)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    int f = 0;
    if (state[i] == UNDECIDED) {
        int best = t1[i];
        if (!in_range(n, best)) best = -1;
        for (int k = Gp[i]; k < Gp[i + 1]; ++k) {
            const int j = Gj[k];
            if (!in_range(n, j)) continue;
            const int c = t1[j];
            if (in_range(n, c) && c != best && exceeds(c, best, Gp)) best = c;
        }
        f = best == i ? 1 : 0;
    }
    flag[i] = f;
}

__global__ void __launch_bounds__(kB) mis2_c1_kernel(int n, const int *Gp, const int *Gj, const int *state, const int *flag,
                                                     int *c1)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    int c = 0;
    if (state[i] != ISOLATED) {
        c = flag[i];
        for (int k = Gp[i]; !c && k < Gp[i + 1]; ++k) {
            const int j = Gj[k];
            if (in_range(n, j) && flag[j]) c = 1;
        }
    }
    c1[i] = c;
}

__global__ void __launch_bounds__(kB) mis2_update_kernel(int n, const int *Gp, const int *Gj, const int *flag, const int *c1,
                                                         int *state, int *is_root, int *block_undecided)
{
    __shared__ int s_red[kB / LMG_WAVE];
    const int i = blockIdx.x * kB + threadIdx.x;
    int und = 0;
    if (i < n) {
        int st = state[i];
        if (st == UNDECIDED) {
            if (flag[i]) st = ROOT;
            else if (c1[i]) st = COVERED;
            else
                for (int k = Gp[i]; k < Gp[i + 1]; ++k) {
                    const int j = Gj[k];
                    if (in_range(n, j) && c1[j]) {
                        st = COVERED;
                        break;
                    }
                }
            state[i] = st;
        }
        is_root[i] = st == ROOT ? 1 : 0;
        und = st == UNDECIDED ? 1 : 0;
    }
#pragma unroll
    for (int off = LMG_WAVE / 2; off > 0; off >>= 1) und += __shfl_down(und, off, LMG_WAVE);
    if ((threadIdx.x & (LMG_WAVE - 1)) == 0) s_red[threadIdx.x / LMG_WAVE] = und;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < kB / LMG_WAVE; ++w) tot += s_red[w];
        block_undecided[blockIdx.x] = tot;
    }
}

// ---- aggregates ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kB) assign1_kernel(int n, const int *Gp, const int *Gj, const int *state, const int *rank,
                                                     int *a1)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const int st = state[i];
    int best = st == ROOT ? i : -1;
    if (st == COVERED)
        for (int k = Gp[i]; k < Gp[i + 1]; ++k) {
            const int j = Gj[k];
            if (in_range(n, j) && state[j] == ROOT && exceeds(j, best, Gp)) best = j;
        }
    a1[i] = best >= 0 ? rank[best] : -1;
}

__global__ void __launch_bounds__(kB) assign2_kernel(int n, const int *Gp, const int *Gj, const int *state, const int *a1,
                                                     int *a2)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    int a = a1[i];
    if (a < 0 && state[i] != ISOLATED) {
        int best = -1;
        for (int k = Gp[i]; k < Gp[i + 1]; ++k) {
            const int j = Gj[k];
            if (in_range(n, j) && a1[j] >= 0 && exceeds(j, best, Gp)) best = j;
        }
        if (best >= 0) a = a1[best];
    }
    a2[i] = a;
}

// ---- the tentative prolongator --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kB) tentative_count_kernel(int n, int n_agg, const int *agg, int *rownnz)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    rownnz[i] = in_range(n_agg, agg[i]) ? 1 : 0;
}

__global__ void __launch_bounds__(kB) tentative_pattern_kernel(int n, int n_agg, const int *agg, const double *B, const int *Tp,
                                                               int *Tj, double *Tv)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const int at = Tp[i];
    if (in_range(n_agg, agg[i]) && at < Tp[i + 1]) {
        Tj[at] = agg[i];
        Tv[at] = B[i];
    }
}

// M: the transpose of the pattern above -- row j lists the members of aggregate j with their B.
__global__ void __launch_bounds__(kB) norms_kernel(int n_agg, const int *Mp, const int *Mj, const double *Mv, double *Bc,
                                                   unsigned long long *status)
{
    const int j = blockIdx.x * kB + threadIdx.x;
    if (j >= n_agg) return;
    const int s0 = Mp[j], e0 = Mp[j + 1];
    double s = 0.0;
    bool ascending = true;
    for (int k = s0; k < e0; ++k) {
        const double b = Mv[k];
        s = s + b * b;
        if (k > s0 && Mj[k] <= Mj[k - 1]) ascending = false;
    }
    Bc[j] = sqrt(s);
    if (!ascending) refuse(status, j, LMG_AMG_MEMBERS);
    else if (s == 0.0 || !isfinite(s)) refuse(status, e0 > s0 ? Mj[s0] : 0, LMG_AMG_CANDIDATE);
}

__global__ void __launch_bounds__(kB) tentative_fill_kernel(int n, int n_agg, const int *agg, const double *B, const double *Bc,
                                                            const int *Tp, double *Tv)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const int a = agg[i], at = Tp[i];
    if (in_range(n_agg, a) && at < Tp[i + 1]) Tv[at] = B[i] / Bc[a];
}

// the states the Jacobi step of amg.hip reads: a row of T with an entry is FINE, an empty one FINE0
__global__ void __launch_bounds__(kB) row_states_kernel(int n, const int *Tp, int *state)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    state[i] = Tp[i + 1] > Tp[i] ? LMG_AMG_FINE : LMG_AMG_FINE0;
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + kB - 1) / kB); }
inline bool rows_ok(int64_t n) { return n >= 0 && n < INT32_MAX - kB; }
inline bool unit(double v) { return v >= 0.0 && v <= 1.0; }

}  // namespace

#define SA_LAUNCH(kernel, rows, ...)                                                   \
    do {                                                                               \
        if ((rows) == 0) return LMG_OK;                                                \
        kernel<<<blocks(rows), kB, 0, lmg_stream(stream)>>>(__VA_ARGS__);              \
        LMG_CHECK_LAUNCH();                                                            \
        return LMG_OK;                                                                 \
    } while (0)

extern "C" {

int lmg_sa_diagonal(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, double *diag, void *stream)
{
    if (!rows_ok(n) || !rowptr || !colidx || !vals || !diag) return LMG_ERR_ARG;
    SA_LAUNCH(diagonal_kernel, n, (int)n, rowptr, colidx, vals, diag);
}

int lmg_sa_strength_count(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, const double *diag,
                          double theta, int32_t *rownnz, void *stream)
{
    if (!rows_ok(n) || !rowptr || !colidx || !vals || !diag || !rownnz || !unit(theta)) return LMG_ERR_ARG;
    SA_LAUNCH(strength_count_kernel, n, (int)n, rowptr, colidx, vals, diag, theta, rownnz);
}

int lmg_sa_strength_fill(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, const double *diag,
                         double theta, const int32_t *s_rowptr, int32_t *s_colidx, void *stream)
{
    if (!rows_ok(n) || !rowptr || !colidx || !vals || !diag || !s_rowptr || !s_colidx || !unit(theta)) return LMG_ERR_ARG;
    SA_LAUNCH(strength_fill_kernel, n, (int)n, rowptr, colidx, vals, diag, theta, s_rowptr, s_colidx);
}

int lmg_sa_graph_count(int64_t n, const int32_t *s_rowptr, const int32_t *s_colidx, const int32_t *st_rowptr,
                       const int32_t *st_colidx, int32_t *rownnz, void *stream)
{
    if (!rows_ok(n) || !s_rowptr || !s_colidx || !st_rowptr || !st_colidx || !rownnz) return LMG_ERR_ARG;
    SA_LAUNCH(graph_count_kernel, n, (int)n, s_rowptr, s_colidx, st_rowptr, st_colidx, rownnz);
}

int lmg_sa_graph_fill(int64_t n, const int32_t *s_rowptr, const int32_t *s_colidx, const int32_t *st_rowptr,
                      const int32_t *st_colidx, const int32_t *g_rowptr, int32_t *g_colidx, void *stream)
{
    if (!rows_ok(n) || !s_rowptr || !s_colidx || !st_rowptr || !st_colidx || !g_rowptr || !g_colidx) return LMG_ERR_ARG;
    SA_LAUNCH(graph_fill_kernel, n, (int)n, s_rowptr, s_colidx, st_rowptr, st_colidx, g_rowptr, g_colidx);
}

int lmg_sa_mis2_init(int64_t n, const int32_t *s_rowptr, int32_t *state, int32_t *is_root, void *stream)
{
    if (!rows_ok(n) || !s_rowptr || !state || !is_root) return LMG_ERR_ARG;
    SA_LAUNCH(mis2_init_kernel, n, (int)n, s_rowptr, state, is_root);
}

int lmg_sa_mis2_t1(int64_t n, const int32_t *g_rowptr, const int32_t *g_colidx, const int32_t *state, int32_t *t1, void *stream)
{
    if (!rows_ok(n) || !g_rowptr || !g_colidx || !state || !t1) return LMG_ERR_ARG;
    SA_LAUNCH(mis2_t1_kernel, n, (int)n, g_rowptr, g_colidx, state, t1);
}

int lmg_sa_mis2_t2(int64_t n, const int32_t *g_rowptr, const int32_t *g_colidx, const int32_t *state, const int32_t *t1,
                   int32_t *flag, void *stream)
{
    if (!rows_ok(n) || !g_rowptr || !g_colidx || !state || !t1 || !flag) return LMG_ERR_ARG;
    SA_LAUNCH(mis2_t2_kernel, n, (int)n, g_rowptr, g_colidx, state, t1, flag);
}

int lmg_sa_mis2_c1(int64_t n, const int32_t *g_rowptr, const int32_t *g_colidx, const int32_t *state, const int32_t *flag,
                   int32_t *c1, void *stream)
{
    if (!rows_ok(n) || !g_rowptr || !g_colidx || !state || !flag || !c1) return LMG_ERR_ARG;
    SA_LAUNCH(mis2_c1_kernel, n, (int)n, g_rowptr, g_colidx, state, flag, c1);
}

int64_t lmg_sa_blocks(int64_t n) { return n > 0 ? (n + kB - 1) / kB : 0; }

int lmg_sa_mis2_update(int64_t n, const int32_t *g_rowptr, const int32_t *g_colidx, const int32_t *flag, const int32_t *c1,
                       int32_t *state, int32_t *is_root, int32_t *block_undecided, void *stream)
{
    if (!rows_ok(n) || !g_rowptr || !g_colidx || !flag || !c1 || !state || !is_root || !block_undecided) return LMG_ERR_ARG;
    SA_LAUNCH(mis2_update_kernel, n, (int)n, g_rowptr, g_colidx, flag, c1, state, is_root, block_undecided);
}

int lmg_sa_assign1(int64_t n, const int32_t *g_rowptr, const int32_t *g_colidx, const int32_t *state, const int32_t *rank,
                   int32_t *a1, void *stream)
{
    if (!rows_ok(n) || !g_rowptr || !g_colidx || !state || !rank || !a1) return LMG_ERR_ARG;
    SA_LAUNCH(assign1_kernel, n, (int)n, g_rowptr, g_colidx, state, rank, a1);
}

int lmg_sa_assign2(int64_t n, const int32_t *g_rowptr, const int32_t *g_colidx, const int32_t *state, const int32_t *a1,
                   int32_t *a2, void *stream)
{
    if (!rows_ok(n) || !g_rowptr || !g_colidx || !state || !a1 || !a2 || a1 == a2) return LMG_ERR_ARG;
    SA_LAUNCH(assign2_kernel, n, (int)n, g_rowptr, g_colidx, state, a1, a2);
}

int lmg_sa_tentative_count(int64_t n, int64_t n_agg, const int32_t *agg, int32_t *rownnz, void *stream)
{
    if (!rows_ok(n) || n_agg < 0 || n_agg > n || !agg || !rownnz) return LMG_ERR_ARG;
    SA_LAUNCH(tentative_count_kernel, n, (int)n, (int)n_agg, agg, rownnz);
}

int lmg_sa_tentative_pattern(int64_t n, int64_t n_agg, const int32_t *agg, const double *cand, const int32_t *t_rowptr,
                             int32_t *t_colidx, double *t_vals, void *stream)
{
    if (!rows_ok(n) || n_agg < 0 || n_agg > n || !agg || !cand || !t_rowptr || !t_colidx || !t_vals) return LMG_ERR_ARG;
    SA_LAUNCH(tentative_pattern_kernel, n, (int)n, (int)n_agg, agg, cand, t_rowptr, t_colidx, t_vals);
}

int lmg_sa_norms(int64_t n_agg, const int32_t *m_rowptr, const int32_t *m_colidx, const double *m_vals, double *coarse_cand,
                 uint64_t *status, void *stream)
{
    if (!rows_ok(n_agg) || !m_rowptr || !m_colidx || !m_vals || !coarse_cand || !status) return LMG_ERR_ARG;
    SA_LAUNCH(norms_kernel, n_agg, (int)n_agg, m_rowptr, m_colidx, m_vals, coarse_cand, (unsigned long long *)status);
}

int lmg_sa_tentative_fill(int64_t n, int64_t n_agg, const int32_t *agg, const double *cand, const double *coarse_cand,
                          const int32_t *t_rowptr, double *t_vals, void *stream)
{
    if (!rows_ok(n) || n_agg < 0 || n_agg > n || !agg || !cand || !coarse_cand || !t_rowptr || !t_vals) return LMG_ERR_ARG;
    SA_LAUNCH(tentative_fill_kernel, n, (int)n, (int)n_agg, agg, cand, coarse_cand, t_rowptr, t_vals);
}

int lmg_sa_row_states(int64_t n, const int32_t *t_rowptr, int32_t *state, void *stream)
{
    if (!rows_ok(n) || !t_rowptr || !state) return LMG_ERR_ARG;
    SA_LAUNCH(row_states_kernel, n, (int)n, t_rowptr, state);
}

}  // extern "C"
