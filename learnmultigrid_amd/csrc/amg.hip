// Classical AMG setup on the device (amg.py): from a matrix A to a prolongation P with nothing else given.  What the reference's
// experiment scripts get from pyamg.ruge_stuben_solver on the host, stage by stage, with a split that runs in parallel (PMIS
// in place of Ruge-Stueben's two sequential passes).  The rules: DESIGN.md section 3, "Classical AMG setup"; the plain-Python
// restatement the kernels are compared with bit for bit: tests/amg_ref.py.
//   - strength count / fill:  one lane per row.  m_ij = -sign(a_ii) a_ij for j != i; entry j is strong iff m_ij > 0 and
//             m_ij >= theta * max_k m_ik.  S keeps the strong columns in A's order; a row with no (or a zero) diagonal has none;
//   - pmis keys:    the first integer of a node's key (its column count in S, the row length of S^T) and the first state:
//             a row of S without entries is FINE0 at once, every other node is undecided;
//   - pmis select:  every undecided node whose key (count, hash(i), i) exceeds that of every undecided neighbour in
//             S_i and S^T_i is flagged: reads states, writes its own flag;
//   - pmis update:  a flagged node becomes coarse, another undecided node with a flagged j in S_i becomes fine: reads flags,
//             writes its own state; the undecided nodes left are counted per workgroup (the host reads their sum, one count per
//             round, and launches the next round);
//   - interp count / fill:  direct interpolation.  A coarse row is one 1.0 at the node's rank; a fine row i has the columns
//             rank[j], j in C_i = S_i and coarse, with -alpha_i a_ij / d_i (S_i is a subsequence of A's row: one walk reads both);
//   - smooth count / fill:  one Jacobi step on P with truncation.  A fine row takes the pattern of (A P)_i, the sorted rows
//             of P and A P are merged, entries below trunc * max leave and the rest is scaled to the row sum before.
// Every kernel owns its rows: no atomics but the refusal of a pivot, which reports (row << 8 | rule) with an atomic minimum on
// one 64-bit status word like nmg2d.hip.  Nothing waits for another workgroup.  No local arrays: no scratch.
#include "lmg_common.hpp"

namespace {

constexpr int kB = 256;
enum { UNDECIDED = LMG_AMG_UNDECIDED, COARSE = LMG_AMG_COARSE, FINE = LMG_AMG_FINE, FINE0 = LMG_AMG_FINE0 };

__device__ __forceinline__ void refuse(unsigned long long *status, long long order, int rule)
{
    atomicMin(status, ((unsigned long long)order << 8) | (unsigned long long)rule);
}

// the stored diagonal of row i, 0.0 where there is none
__device__ __forceinline__ double diagonal_of(int i, const int *Ap, const int *Aj, const double *Av)
{
    double d = 0.0;
    for (int k = Ap[i]; k < Ap[i + 1]; ++k)
        if (Aj[k] == i) d = Av[k];
    return d;
}

// ---- strength ---------------------------------------------------------------------------------------------------------
// The threshold of row i: theta * max m, or a negative number where the row has no strong entry.  neg: a_ii < 0.
__device__ __forceinline__ double strength_threshold(int n, int i, const int *Ap, const int *Aj, const double *Av, double theta,
                                                     bool &neg)
{
    const double d = diagonal_of(i, Ap, Aj, Av);
    neg = d < 0.0;
    if (!(d != 0.0)) return -1.0;
    double mx = 0.0;
    for (int k = Ap[i]; k < Ap[i + 1]; ++k) {
        const int j = Aj[k];
        const double m = neg ? Av[k] : -Av[k];
        if (j != i && (unsigned)j < (unsigned)n && m > mx) mx = m;
    }
    if (!(mx > 0.0)) return -1.0;
    return theta * mx;
}

__device__ __forceinline__ bool is_strong(int n, int i, int j, double v, bool neg, double thr)
{
    const double m = neg ? v : -v;
    return j != i && (unsigned)j < (unsigned)n && m > 0.0 && m >= thr;
}

__global__ void __launch_bounds__(kB) strength_count_kernel(int n, const int *Ap, const int *Aj, const double *Av, double theta,
                                                            int *rownnz)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    bool neg;
    const double thr = strength_threshold(n, i, Ap, Aj, Av, theta, neg);
    int c = 0;
    if (thr >= 0.0)
        for (int k = Ap[i]; k < Ap[i + 1]; ++k) c += is_strong(n, i, Aj[k], Av[k], neg, thr) ? 1 : 0;
    rownnz[i] = c;
}

__global__ void __launch_bounds__(kB) strength_fill_kernel(int n, const int *Ap, const int *Aj, const double *Av, double theta,
                                                           const int *Sp, int *Sj)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    bool neg;
    const double thr = strength_threshold(n, i, Ap, Aj, Av, theta, neg);
    if (!(thr >= 0.0)) return;
    int at = Sp[i];
    const int end = Sp[i + 1];
    for (int k = Ap[i]; k < Ap[i + 1]; ++k)
        if (is_strong(n, i, Aj[k], Av[k], neg, thr) && at < end) Sj[at++] = Aj[k];
}

// ---- PMIS -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned hash32(unsigned x)
{
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

__global__ void __launch_bounds__(kB) pmis_keys_kernel(int n, const int *Sp, const int *STp, int *count, int *state, int *is_coarse)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    count[i] = STp[i + 1] - STp[i];
    state[i] = Sp[i + 1] > Sp[i] ? UNDECIDED : FINE0;
    is_coarse[i] = 0;
}

// whether the key of i does not exceed the key of an undecided j (then i is not flagged this round)
__device__ __forceinline__ bool beaten(int n, int i, int ci, unsigned hi, int j, const int *count, const int *state)
{
    if (j == i || (unsigned)j >= (unsigned)n || state[j] != UNDECIDED) return false;
    const int cj = count[j];
    if (ci != cj) return ci < cj;
    const unsigned hj = hash32((unsigned)j);
    if (hi != hj) return hi < hj;
    return i < j;
}

__global__ void __launch_bounds__(kB) pmis_select_kernel(int n, const int *Sp, const int *Sj, const int *STp, const int *STj,
                                                         const int *count, const int *state, int *flag)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    int f = 0;
    if (state[i] == UNDECIDED) {
        const int ci = count[i];
        const unsigned hi = hash32((unsigned)i);
        f = 1;
        for (int k = Sp[i]; f && k < Sp[i + 1]; ++k)
            if (beaten(n, i, ci, hi, Sj[k], count, state)) f = 0;
        for (int k = STp[i]; f && k < STp[i + 1]; ++k)
            if (beaten(n, i, ci, hi, STj[k], count, state)) f = 0;
    }
    flag[i] = f;
}

__global__ void __launch_bounds__(kB) pmis_update_kernel(int n, const int *Sp, const int *Sj, const int *flag, int *state,
                                                         int *is_coarse, int *block_undecided)
{
    __shared__ int s_red[kB / LMG_WAVE];
    const int i = blockIdx.x * kB + threadIdx.x;
    int und = 0;
    if (i < n) {
        int st = state[i];
        if (st == UNDECIDED) {
            if (flag[i]) st = COARSE;
            else
                for (int k = Sp[i]; k < Sp[i + 1]; ++k) {
                    const int j = Sj[k];
                    if ((unsigned)j < (unsigned)n && flag[j]) {
                        st = FINE;
                        break;
                    }
                }
            state[i] = st;
        }
        is_coarse[i] = st == COARSE ? 1 : 0;
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

// ---- direct interpolation -----------------------------------------------------------------------------------------------
__device__ __forceinline__ bool coarse_at(int n, int j, const int *state) { return (unsigned)j < (unsigned)n && state[j] == COARSE; }

__global__ void __launch_bounds__(kB) interp_count_kernel(int n, const int *Sp, const int *Sj, const int *state, int *rownnz)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const int st = state[i];
    int c = st == COARSE ? 1 : 0;
    if (st == FINE)
        for (int k = Sp[i]; k < Sp[i + 1]; ++k) c += coarse_at(n, Sj[k], state) ? 1 : 0;
    rownnz[i] = c;
}

__global__ void __launch_bounds__(kB) interp_fill_kernel(int n, const int *Ap, const int *Aj, const double *Av, const int *Sp,
                                                         const int *Sj, const int *state, const int *rank, const int *Pp,
                                                         int *Pj, double *Pv, unsigned long long *status)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const int st = state[i];
    int at = Pp[i];
    const int end = Pp[i + 1];
    if (st == COARSE) {
        if (at < end) {
            Pj[at] = rank[i];
            Pv[at] = 1.0;
        }
        return;
    }
    if (st != FINE || at >= end) return;
    // one walk over the row: the diagonal, the two sums of the off-diagonal entries by sign, the sum over C_i
    double aii = 0.0, same = 0.0, other = 0.0, csum = 0.0;
    const double d0 = diagonal_of(i, Ap, Aj, Av);
    const bool neg = d0 < 0.0;
    int t = Sp[i];
    const int tend = Sp[i + 1];
    for (int k = Ap[i]; k < Ap[i + 1]; ++k) {
        const int j = Aj[k];
        const double v = Av[k];
        if (j == i) aii = v;
        else if (neg ? v < 0.0 : v > 0.0) same = same + v;
        else if (neg ? v > 0.0 : v < 0.0) other = other + v;
        if (t < tend && Sj[t] == j) {
            ++t;
            if (coarse_at(n, j, state)) csum = csum + v;
        }
    }
    const double d = aii + same;
    if (d == 0.0 || !isfinite(d)) {
        refuse(status, i, LMG_AMG_PIVOT);
        return;
    }
    const double alpha = other / csum;
    t = Sp[i];
    for (int k = Ap[i]; k < Ap[i + 1]; ++k) {
        const int j = Aj[k];
        if (t < tend && Sj[t] == j) {
            ++t;
            if (coarse_at(n, j, state) && at < end) {
                Pj[at] = rank[j];
                Pv[at] = -(alpha * Av[k]) / d;
                ++at;
            }
        }
    }
}

// ---- one Jacobi step on P, truncated ------------------------------------------------------------------------------------
// Row i of the step before truncation, entry by entry in the order of (A P)_i: f(column, value), value = P_ic - (omega AP_ic) / a_ii
// with P_ic = 0 where P has no such entry.  Both rows have ascending columns.
template <typename F>
__device__ __forceinline__ void smoothed_row(int i, double aii, double omega, const int *Pp, const int *Pj, const double *Pv,
                                             const int *Xp, const int *Xj, const double *Xv, F &&f)
{
    int p = Pp[i];
    const int pend = Pp[i + 1];
    for (int k = Xp[i]; k < Xp[i + 1]; ++k) {
        const int c = Xj[k];
        while (p < pend && Pj[p] < c) ++p;
        const double old = (p < pend && Pj[p] == c) ? Pv[p] : 0.0;
        f(c, old - (omega * Xv[k]) / aii);
    }
}

struct SmoothArgs {
    int n;
    const int *Ap, *Aj;
    const double *Av;
    const int *Pp, *Pj;
    const double *Pv;
    const int *Xp, *Xj;
    const double *Xv;
    const int *state, *rank;
    double omega, trunc;
};

__global__ void __launch_bounds__(kB) smooth_count_kernel(SmoothArgs a, int *rownnz)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= a.n) return;
    const int st = a.state[i];
    int c = st == COARSE ? 1 : 0;
    if (st == FINE) {
        const double aii = diagonal_of(i, a.Ap, a.Aj, a.Av);
        double mx = 0.0;
        smoothed_row(i, aii, a.omega, a.Pp, a.Pj, a.Pv, a.Xp, a.Xj, a.Xv, [&](int, double v) {
            if (fabs(v) > mx) mx = fabs(v);
        });
        const double thr = a.trunc * mx;
        smoothed_row(i, aii, a.omega, a.Pp, a.Pj, a.Pv, a.Xp, a.Xj, a.Xv, [&](int, double v) { c += fabs(v) < thr ? 0 : 1; });
    }
    rownnz[i] = c;
}

__global__ void __launch_bounds__(kB) smooth_fill_kernel(SmoothArgs a, const int *Qp, int *Qj, double *Qv)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= a.n) return;
    const int st = a.state[i];
    int at = Qp[i];
    const int end = Qp[i + 1];
    if (st == COARSE) {
        if (at < end) {
            Qj[at] = a.rank[i];
            Qv[at] = 1.0;
        }
        return;
    }
    if (st != FINE) return;
    const double aii = diagonal_of(i, a.Ap, a.Aj, a.Av);
    double mx = 0.0;
    smoothed_row(i, aii, a.omega, a.Pp, a.Pj, a.Pv, a.Xp, a.Xj, a.Xv, [&](int, double v) {
        if (fabs(v) > mx) mx = fabs(v);
    });
    const double thr = a.trunc * mx;
    double before = 0.0, after = 0.0;
    smoothed_row(i, aii, a.omega, a.Pp, a.Pj, a.Pv, a.Xp, a.Xj, a.Xv, [&](int, double v) {
        before = before + v;
        if (!(fabs(v) < thr)) after = after + v;
    });
    const bool rescale = after != 0.0;
    const double scale = rescale ? before / after : 1.0;
    smoothed_row(i, aii, a.omega, a.Pp, a.Pj, a.Pv, a.Xp, a.Xj, a.Xv, [&](int c, double v) {
        if (!(fabs(v) < thr) && at < end) {
            Qj[at] = c;
            Qv[at] = rescale ? v * scale : v;
            ++at;
        }
    });
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + kB - 1) / kB); }
inline bool rows_ok(int64_t n) { return n >= 0 && n < INT32_MAX - kB; }

}  // namespace

extern "C" {

int lmg_amg_strength_count(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, double theta,
                           int32_t *rownnz, void *stream)
{
    if (!rows_ok(n) || !rowptr || !colidx || !vals || !rownnz || !(theta >= 0.0 && theta <= 1.0)) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    strength_count_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, rowptr, colidx, vals, theta, rownnz);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_amg_strength_fill(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, double theta,
                          const int32_t *s_rowptr, int32_t *s_colidx, void *stream)
{
    if (!rows_ok(n) || !rowptr || !colidx || !vals || !s_rowptr || !s_colidx || !(theta >= 0.0 && theta <= 1.0))
        return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    strength_fill_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, rowptr, colidx, vals, theta, s_rowptr, s_colidx);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_amg_pmis_keys(int64_t n, const int32_t *s_rowptr, const int32_t *st_rowptr, int32_t *count, int32_t *state,
                      int32_t *is_coarse, void *stream)
{
    if (!rows_ok(n) || !s_rowptr || !st_rowptr || !count || !state || !is_coarse) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    pmis_keys_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, s_rowptr, st_rowptr, count, state, is_coarse);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_amg_pmis_select(int64_t n, const int32_t *s_rowptr, const int32_t *s_colidx, const int32_t *st_rowptr,
                        const int32_t *st_colidx, const int32_t *count, const int32_t *state, int32_t *flag, void *stream)
{
    if (!rows_ok(n) || !s_rowptr || !s_colidx || !st_rowptr || !st_colidx || !count || !state || !flag) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    pmis_select_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, s_rowptr, s_colidx, st_rowptr, st_colidx, count, state,
                                                                 flag);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int64_t lmg_amg_pmis_blocks(int64_t n) { return n > 0 ? (n + kB - 1) / kB : 0; }

int lmg_amg_pmis_update(int64_t n, const int32_t *s_rowptr, const int32_t *s_colidx, const int32_t *flag, int32_t *state,
                        int32_t *is_coarse, int32_t *block_undecided, void *stream)
{
    if (!rows_ok(n) || !s_rowptr || !s_colidx || !flag || !state || !is_coarse || !block_undecided) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    pmis_update_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, s_rowptr, s_colidx, flag, state, is_coarse,
                                                                 block_undecided);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_amg_interp_count(int64_t n, const int32_t *s_rowptr, const int32_t *s_colidx, const int32_t *state, int32_t *rownnz,
                         void *stream)
{
    if (!rows_ok(n) || !s_rowptr || !s_colidx || !state || !rownnz) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    interp_count_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, s_rowptr, s_colidx, state, rownnz);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_amg_interp_fill(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, const int32_t *s_rowptr,
                        const int32_t *s_colidx, const int32_t *state, const int32_t *rank, const int32_t *p_rowptr,
                        int32_t *p_colidx, double *p_vals, uint64_t *status, void *stream)
{
    if (!rows_ok(n) || !rowptr || !colidx || !vals || !s_rowptr || !s_colidx || !state || !rank || !p_rowptr || !p_colidx ||
        !p_vals || !status)
        return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    interp_fill_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, rowptr, colidx, vals, s_rowptr, s_colidx, state, rank,
                                                                 p_rowptr, p_colidx, p_vals, (unsigned long long *)status);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

static int smooth_args(SmoothArgs &a, int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                       const int32_t *p_rowptr, const int32_t *p_colidx, const double *p_vals, const int32_t *ap_rowptr,
                       const int32_t *ap_colidx, const double *ap_vals, const int32_t *state, const int32_t *rank, double omega,
                       double trunc)
{
    if (!rows_ok(n) || !rowptr || !colidx || !vals || !p_rowptr || !p_colidx || !p_vals || !ap_rowptr || !ap_colidx || !ap_vals ||
        !state || !rank || !std::isfinite(omega) || !(trunc >= 0.0 && trunc <= 1.0))
        return LMG_ERR_ARG;
    a = {(int)n, rowptr, colidx, vals, p_rowptr, p_colidx, p_vals, ap_rowptr, ap_colidx, ap_vals, state, rank, omega, trunc};
    return LMG_OK;
}

int lmg_amg_smooth_count(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, const int32_t *p_rowptr,
                         const int32_t *p_colidx, const double *p_vals, const int32_t *ap_rowptr, const int32_t *ap_colidx,
                         const double *ap_vals, const int32_t *state, const int32_t *rank, double omega, double trunc,
                         int32_t *rownnz, void *stream)
{
    SmoothArgs a;
    if (smooth_args(a, n, rowptr, colidx, vals, p_rowptr, p_colidx, p_vals, ap_rowptr, ap_colidx, ap_vals, state, rank, omega,
                    trunc) != LMG_OK || !rownnz)
        return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    smooth_count_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>(a, rownnz);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_amg_smooth_fill(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, const int32_t *p_rowptr,
                        const int32_t *p_colidx, const double *p_vals, const int32_t *ap_rowptr, const int32_t *ap_colidx,
                        const double *ap_vals, const int32_t *state, const int32_t *rank, double omega, double trunc,
                        const int32_t *q_rowptr, int32_t *q_colidx, double *q_vals, void *stream)
{
    SmoothArgs a;
    if (smooth_args(a, n, rowptr, colidx, vals, p_rowptr, p_colidx, p_vals, ap_rowptr, ap_colidx, ap_vals, state, rank, omega,
                    trunc) != LMG_OK || !q_rowptr || !q_colidx || !q_vals)
        return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    smooth_fill_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>(a, q_rowptr, q_colidx, q_vals);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

}  // extern "C"
