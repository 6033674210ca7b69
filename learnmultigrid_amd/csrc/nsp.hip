// Smoothed aggregation for systems (aggregation.py): node blocks of bs unknowns and a tentative prolongator of k <= 6
// near-nullspace candidates, by two rounds of Cholesky-QR per aggregate.  What pyamg.smoothed_aggregation_solver(A, B) does
// with a BSR matrix and B of shape (n, k).  The rules: DESIGN.md section 3, "Smoothed aggregation for systems"; the
// plain-Python restatement the kernels are compared with bit for bit: tests/nsp_ref.py.
//   - condense count / fill:  one lane per NODE row I of C (N = n / bs rows): the merge of the bs sorted rows bs I .. bs I + bs - 1
//             of A.  An entry (I, J) iff some stored a_ij lies in the block, explicit zeros included; columns ascend;
//             c_IJ = sqrt(sum a_ij a_ij), the sum from 0.0 over the rows of the block ascending and in storage order within a
//             row.  The next node column is found by a binary search in each of the bs rows, so there is no cursor array.
//             Strength, graph, MIS-2 roots and aggregates are the kernels of sa.hip on C;
//   - gram_chol:      one lane per aggregate j on the member list of its nodes (the transpose of lmg_sa_tentative_pattern on
//             the node aggregates: ascending).  g_pq = the sum of x_ip x_iq, p <= q, over the member rows: the nodes ascending,
//             the unknowns within a node ascending.  Then for c = 0 .. k-1 and r = 0 .. c:
//             s = g_rc - R_0r R_0c - ... - R_(r-1)r R_(r-1)c; r < c: R_rc = s / R_rr; r = c: R_cc = sqrt(s), and the aggregate
//             is REFUSED unless s is finite and s > rank_tol g_cc.  R is written as k x k, zeros below the diagonal;
//   - apply:          one lane per unknown i of an aggregated node: y_0 = x_0 / R_00,
//             y_c = (x_c - y_0 R_0c - ... - y_(c-1) R_(c-1)c) / R_cc with the R of the node's aggregate; other rows untouched;
//   - tri_product:    one lane per aggregate: Bc_j = R' R, (R' R)_rc = the sum over q = r .. c of R'_rq R_qc from 0.0, zeros below;
//   - tentative count / fill:  k entries for a row of an aggregated node, else none; after the caller's scan the columns
//             k agg + c, c ascending, with the values of the SECOND application (y R'^-1 as in apply), written straight into T.
// k is a template parameter (1 .. 6, chosen by a switch in the entry point): the Gram sums, R and a row of x are arrays that
// only fully unrolled loops index, so they live in registers -- no scratch.  bs sizes nothing and stays a run-time value.
// Every kernel reads arrays an earlier launch wrote and writes its own lane's entries; no atomics but the refusals, which
// report (row << 8 | rule) with an atomic minimum on one 64-bit status word like sa.hip.  Nothing waits for another workgroup.
#include "lmg_common.hpp"

#include <climits>

namespace {

constexpr int kB = 256;
constexpr int kMaxK = LMG_NSP_MAX_CANDIDATES;

__device__ __forceinline__ void refuse(unsigned long long *status, long long order, int rule)
{
    atomicMin(status, ((unsigned long long)order << 8) | (unsigned long long)rule);
}

__device__ __forceinline__ bool in_range(int n, int j) { return (unsigned)j < (unsigned)n; }

// ---- condensation ---------------------------------------------------------------------------------------------------------
// the first position in [lo, hi) of the ascending Aj with Aj[pos] >= target
__device__ __forceinline__ int lower_bound(const int *Aj, int lo, int hi, int target)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (Aj[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// f(J, position of its first entry per row is searched again by the caller): every node column of node row I, ascending
template <typename F>
__device__ __forceinline__ void node_columns(int N, int bs, int I, const int *Ap, const int *Aj, F &&f)
{
    const int n = N * bs;
    int cur = -1;
    for (;;) {
        int next = INT_MAX;
        const int target = (cur + 1) * bs;
        for (int r = 0; r < bs; ++r) {
            const int row = bs * I + r, end = Ap[row + 1];
            const int at = lower_bound(Aj, Ap[row], end, target);
            if (at < end) {
                const int j = Aj[at];
                if (in_range(n, j) && j / bs > cur && j / bs < next) next = j / bs;
            }
        }
        if (next == INT_MAX) return;
        f(next);
        cur = next;
    }
}

__global__ void __launch_bounds__(kB) condense_count_kernel(int N, int bs, const int *Ap, const int *Aj, int *rownnz)
{
    const int I = blockIdx.x * kB + threadIdx.x;
    if (I >= N) return;
    int c = 0;
    node_columns(N, bs, I, Ap, Aj, [&](int) { ++c; });
    rownnz[I] = c;
}

__global__ void __launch_bounds__(kB) condense_fill_kernel(int N, int bs, const int *Ap, const int *Aj, const double *Av,
                                                           const int *Cp, int *Cj, double *Cv)
{
    const int I = blockIdx.x * kB + threadIdx.x;
    if (I >= N) return;
    int at = Cp[I];
    const int end = Cp[I + 1];
    node_columns(N, bs, I, Ap, Aj, [&](int J) {
        double s = 0.0;
        for (int r = 0; r < bs; ++r) {
            const int row = bs * I + r, e = Ap[row + 1];
            for (int k = lower_bound(Aj, Ap[row], e, J * bs); k < e && Aj[k] < J * bs + bs; ++k) s = s + Av[k] * Av[k];
        }
        if (at < end) {
            Cj[at] = J;
            Cv[at] = sqrt(s);
            ++at;
        }
    });
}

// ---- Cholesky-QR per aggregate ------------------------------------------------------------------------------------------
// M: row j lists the member NODES of aggregate j, ascending.  X: n x K, row-major.  R: n_agg x K x K.
template <int K>
__global__ void __launch_bounds__(kB) gram_chol_kernel(int n_agg, int N, int bs, const int *Mp, const int *Mj, const double *X,
                                                       double rank_tol, double *R, unsigned long long *status)
{
    const int j = blockIdx.x * kB + threadIdx.x;
    if (j >= n_agg) return;
    double g[K][K], f[K][K];
#pragma unroll
    for (int p = 0; p < K; ++p)
#pragma unroll
        for (int q = 0; q < K; ++q) g[p][q] = 0.0, f[p][q] = 0.0;
    const int s0 = Mp[j], e0 = Mp[j + 1];
    bool ascending = true;
    for (int m = s0; m < e0; ++m) {
        const int node = Mj[m];
        if (m > s0 && node <= Mj[m - 1]) ascending = false;
        if (!in_range(N, node)) continue;
        for (int u = 0; u < bs; ++u) {
            const double *xr = X + ((size_t)node * bs + u) * K;
            double x[K];
#pragma unroll
            for (int p = 0; p < K; ++p) x[p] = xr[p];
#pragma unroll
            for (int p = 0; p < K; ++p)
#pragma unroll
                for (int q = p; q < K; ++q) g[p][q] = g[p][q] + x[p] * x[q];
        }
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < K; ++c)
#pragma unroll
        for (int r = 0; r <= c; ++r) {
            double s = g[r][c];
#pragma unroll
            for (int q = 0; q < r; ++q) s = s - f[q][r] * f[q][c];
            if (r < c) f[r][c] = s / f[r][r];
            else {
                if (!(isfinite(s) && s > rank_tol * g[c][c])) ok = false;
                f[c][c] = sqrt(s);
            }
        }
    double *Rj = R + (size_t)j * (K * K);
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int c = 0; c < K; ++c) Rj[r * K + c] = f[r][c];
    if (!ascending) refuse(status, j, LMG_AMG_MEMBERS);
    else if (!ok) refuse(status, e0 > s0 ? (long long)Mj[s0] * bs : 0, LMG_AMG_CANDIDATE);
}

// y = x R^-1 for the row xr and the factor Rj (K x K, upper)
template <int K>
__device__ __forceinline__ void solve_row(const double *xr, const double *Rj, double (&y)[K])
{
    double f[K][K], x[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        x[c] = xr[c];
#pragma unroll
        for (int q = 0; q <= c; ++q) f[q][c] = Rj[q * K + c];
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        double t = x[c];
#pragma unroll
        for (int q = 0; q < c; ++q) t = t - y[q] * f[q][c];
        y[c] = t / f[c][c];
    }
}

template <int K>
__global__ void __launch_bounds__(kB) apply_kernel(int n, int n_agg, int bs, const int *agg, const double *X, const double *R,
                                                   double *Y)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const int a = agg[i / bs];
    if (!in_range(n_agg, a)) return;
    double y[K];
    solve_row<K>(X + (size_t)i * K, R + (size_t)a * (K * K), y);
#pragma unroll
    for (int c = 0; c < K; ++c) Y[(size_t)i * K + c] = y[c];
}

template <int K>
__global__ void __launch_bounds__(kB) tri_product_kernel(int n_agg, const double *R2, const double *R1, double *Bc)
{
    const int j = blockIdx.x * kB + threadIdx.x;
    if (j >= n_agg) return;
    const double *a = R2 + (size_t)j * (K * K), *b = R1 + (size_t)j * (K * K);
    double *out = Bc + (size_t)j * (K * K);
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int c = 0; c < K; ++c) {
            double s = 0.0;
#pragma unroll
            for (int q = r; q <= c; ++q) s = s + a[r * K + q] * b[q * K + c];
            out[r * K + c] = s;
        }
}

__global__ void __launch_bounds__(kB) tentative_count_kernel(int n, int n_agg, int bs, int k, const int *agg, int *rownnz)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    rownnz[i] = in_range(n_agg, agg[i / bs]) ? k : 0;
}

template <int K>
__global__ void __launch_bounds__(kB) tentative_fill_kernel(int n, int n_agg, int bs, const int *agg, const double *Y,
                                                            const double *R2, const int *Tp, int *Tj, double *Tv)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const int a = agg[i / bs], at = Tp[i];
    if (!in_range(n_agg, a) || Tp[i + 1] - at < K) return;
    double y[K];
    solve_row<K>(Y + (size_t)i * K, R2 + (size_t)a * (K * K), y);
#pragma unroll
    for (int c = 0; c < K; ++c) {
        Tj[at + c] = K * a + c;
        Tv[at + c] = y[c];
    }
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + kB - 1) / kB); }
inline bool rows_ok(int64_t n) { return n >= 0 && n < INT32_MAX - kB; }
inline bool k_ok(int32_t k) { return k >= 1 && k <= kMaxK; }
// n unknowns in blocks of bs, n_agg aggregates of nodes, k n_agg coarse unknowns: all within the row limit
inline bool sizes_ok(int64_t n, int64_t n_agg, int32_t bs, int32_t k)
{
    return rows_ok(n) && bs >= 1 && n % bs == 0 && k_ok(k) && n_agg >= 0 && n_agg <= n / bs && rows_ok(n_agg * k);
}

}  // namespace

// one instance per k; `rows` == 0: nothing to do
#define NSP_LAUNCH_K(kernel, k, rows, ...)                                                         \
    do {                                                                                           \
        if ((rows) == 0) return LMG_OK;                                                            \
        switch (k) {                                                                               \
        case 1: kernel<1><<<blocks(rows), kB, 0, lmg_stream(stream)>>>(__VA_ARGS__); break;        \
        case 2: kernel<2><<<blocks(rows), kB, 0, lmg_stream(stream)>>>(__VA_ARGS__); break;        \
        case 3: kernel<3><<<blocks(rows), kB, 0, lmg_stream(stream)>>>(__VA_ARGS__); break;        \
        case 4: kernel<4><<<blocks(rows), kB, 0, lmg_stream(stream)>>>(__VA_ARGS__); break;        \
        case 5: kernel<5><<<blocks(rows), kB, 0, lmg_stream(stream)>>>(__VA_ARGS__); break;        \
        case 6: kernel<6><<<blocks(rows), kB, 0, lmg_stream(stream)>>>(__VA_ARGS__); break;        \
        default: return LMG_ERR_ARG;                                                               \
        }                                                                                          \
        LMG_CHECK_LAUNCH();                                                                        \
        return LMG_OK;                                                                             \
    } while (0)

#define NSP_LAUNCH(kernel, rows, ...)                                                  \
    do {                                                                               \
        if ((rows) == 0) return LMG_OK;                                                \
        kernel<<<blocks(rows), kB, 0, lmg_stream(stream)>>>(__VA_ARGS__);              \
        LMG_CHECK_LAUNCH();                                                            \
        return LMG_OK;                                                                 \
    } while (0)

extern "C" {

int lmg_nsp_condense_count(int64_t n_nodes, int32_t bs, const int32_t *rowptr, const int32_t *colidx, int32_t *rownnz,
                           void *stream)
{
    if (!rows_ok(n_nodes) || bs < 1 || !rows_ok(n_nodes * bs) || !rowptr || !colidx || !rownnz) return LMG_ERR_ARG;
    NSP_LAUNCH(condense_count_kernel, n_nodes, (int)n_nodes, bs, rowptr, colidx, rownnz);
}

int lmg_nsp_condense_fill(int64_t n_nodes, int32_t bs, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                          const int32_t *c_rowptr, int32_t *c_colidx, double *c_vals, void *stream)
{
    if (!rows_ok(n_nodes) || bs < 1 || !rows_ok(n_nodes * bs) || !rowptr || !colidx || !vals || !c_rowptr || !c_colidx
        || !c_vals)
        return LMG_ERR_ARG;
    NSP_LAUNCH(condense_fill_kernel, n_nodes, (int)n_nodes, bs, rowptr, colidx, vals, c_rowptr, c_colidx, c_vals);
}

int lmg_nsp_gram_chol(int64_t n_agg, int64_t n_nodes, int32_t bs, int32_t k, const int32_t *m_rowptr, const int32_t *m_colidx,
                      const double *x, double rank_tol, double *r, uint64_t *status, void *stream)
{
    if (!rows_ok(n_agg) || !rows_ok(n_nodes) || bs < 1 || !sizes_ok(n_nodes * bs, n_agg, bs, k) || !m_rowptr || !m_colidx
        || !x || !r || !status || !(rank_tol > 0.0) || !std::isfinite(rank_tol))
        return LMG_ERR_ARG;
    NSP_LAUNCH_K(gram_chol_kernel, k, n_agg, (int)n_agg, (int)n_nodes, bs, m_rowptr, m_colidx, x, rank_tol, r,
                 (unsigned long long *)status);
}

int lmg_nsp_apply(int64_t n, int64_t n_agg, int32_t bs, int32_t k, const int32_t *agg, const double *x, const double *r,
                  double *y, void *stream)
{
    if (!sizes_ok(n, n_agg, bs, k) || !agg || !x || !r || !y || x == y) return LMG_ERR_ARG;
    NSP_LAUNCH_K(apply_kernel, k, n, (int)n, (int)n_agg, bs, agg, x, r, y);
}

int lmg_nsp_tri_product(int64_t n_agg, int32_t k, const double *r2, const double *r1, double *coarse_cand, void *stream)
{
    if (!rows_ok(n_agg) || !k_ok(k) || !rows_ok(n_agg * k) || !r2 || !r1 || !coarse_cand) return LMG_ERR_ARG;
    NSP_LAUNCH_K(tri_product_kernel, k, n_agg, (int)n_agg, r2, r1, coarse_cand);
}

int lmg_nsp_tentative_count(int64_t n, int64_t n_agg, int32_t bs, int32_t k, const int32_t *agg, int32_t *rownnz, void *stream)
{
    if (!sizes_ok(n, n_agg, bs, k) || !agg || !rownnz) return LMG_ERR_ARG;
    NSP_LAUNCH(tentative_count_kernel, n, (int)n, (int)n_agg, bs, k, agg, rownnz);
}

int lmg_nsp_tentative_fill(int64_t n, int64_t n_agg, int32_t bs, int32_t k, const int32_t *agg, const double *y,
                           const double *r2, const int32_t *t_rowptr, int32_t *t_colidx, double *t_vals, void *stream)
{
    if (!sizes_ok(n, n_agg, bs, k) || !agg || !y || !r2 || !t_rowptr || !t_colidx || !t_vals) return LMG_ERR_ARG;
    NSP_LAUNCH_K(tentative_fill_kernel, k, n, (int)n, (int)n_agg, bs, agg, y, r2, t_rowptr, t_colidx, t_vals);
}

}  // extern "C"
