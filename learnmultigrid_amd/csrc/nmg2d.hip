// The producer of the 2-D learned transfers on the device (NeuralMG_2D.define_hierarchy, learned_q2d.py): what comes
// before and after the caller's model.predict on every level.
//
// learn_multigrid/solvers/Multigrid.py:373-765 does this node by node on lil rows and on dense n x n / n x n_c arrays:
// extract_patches + single_extraction + direct_neighs + intersecting_rows (:456-677) build, per coarse node, the 43
// mass-matrix values the model is shown and the 31 places its 31 answers go to; fill_B (:687-732) folds the answers into a
// dense B; define_hierarchy (:758-759) divides B's rows by their sums; pre_process (:735-739) cuts the coarse mass matrix.
// Here everything reads the sorted CSR arrays of M and nothing dense exists (the rules: DESIGN.md section 3):
//   - check:  one lane per row, the domain of the rules (positive diagonal, no negative off-diagonal entry);
//   - count:  one lane per coarse node, its number of positive neighbours (7: a second patch, 8 and more: refused);
//   - patch:  one lane per patch.  Row c, its <= 6 neighbour rows and their <= 5 x <= 8 second rows are gathers through the
//             CSR arrays (they hit L2: neighbouring patches read the same rows); coarse membership is rank[] >= 0.  The lists
//             a lane keeps are bounded by the rules: 7 neighbours, a 6-slot and an 8-slot window for "while more than 5 / 7
//             remain, delete the first smallest" (deleting the first smallest of every 6 / 8 as the values arrive keeps the
//             same ones: both keep the largest under the order (value, position)), 6 coarse second neighbours, and
//             5 x 7 = 35 candidates for the last-three list;
//   - contrib / fold / normalize / dneighs: every valid slot of every patch is one (key = row * n_c + col, value), the
//             caller sorts the keys stably (patch order inside a key), one lane per distinct entry folds its run in order;
//   - cut_mark / cut_fill: entries of the coarse CSR kept by d_neighs, counted per row, then compacted.
// A refusal never overruns a list: the lane reports (its order << 8 | rule) with an atomic minimum on one 64-bit status
// word and leaves; the host reads the word once per stage, so the FIRST offender in the order of the rules is named.
#include "lmg_common.hpp"

namespace {

constexpr int kB = 256;
constexpr int kPatch = 43, kIdx = 31;

__device__ __forceinline__ void refuse(unsigned long long *status, long long order, int rule)
{
    atomicMin(status, ((unsigned long long)order << 8) | (unsigned long long)rule);
}

// the scaling table by neighbour count m = 2 .. 5 (scaling_vnodes, :429-436)
__device__ __forceinline__ double scale_up(int m) { return m == 2 ? 6.0 : m == 3 ? 3.0 : m == 4 ? 2.0 : 1.5; }
__device__ __forceinline__ double scale_down(int m) { return (double)(m - 1); }

__global__ void __launch_bounds__(kB) check_kernel(int n, const int *Ap, const int *Aj, const double *Av,
                                                   unsigned long long *status)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    double diag = 0.0;
    for (int k = Ap[i]; k < Ap[i + 1]; ++k) {
        const int j = Aj[k];
        const double v = Av[k];
        if (j < 0 || j >= n) {
            refuse(status, i, LMG_NMG2D_COLUMN);
            return;
        }
        if (j == i) diag = v;
        else if (v < 0.0) {
            refuse(status, i, LMG_NMG2D_NEGATIVE);
            return;
        }
    }
    if (!(diag > 0.0)) refuse(status, i, LMG_NMG2D_DIAGONAL);
}

__global__ void __launch_bounds__(kB) count_kernel(int nc, const int *cc, const int *Ap, const int *Aj, const double *Av,
                                                   int *extra, unsigned long long *status)
{
    const int r = blockIdx.x * kB + threadIdx.x;
    if (r >= nc) return;
    const int c = cc[r];
    int k = 0;
    for (int e = Ap[c]; e < Ap[c + 1]; ++e) k += (Aj[e] != c && Av[e] > 0.0) ? 1 : 0;
    if (k >= 8) refuse(status, r, LMG_NMG2D_VALENCE);
    extra[r] = k == 7 ? 1 : 0;
}

// one value more in a window of at most CAP - 1 kept ones: append, and with CAP of them delete the first smallest
template <int CAP>
__device__ __forceinline__ void window_push(double *wv, int *wc, int &q, double v, int col)
{
    wv[q] = v;
    wc[q] = col;
    ++q;
    if (q == CAP) {
        int at = 0;
        for (int t = 1; t < CAP; ++t)
            if (wv[t] < wv[at]) at = t;
        for (int t = at; t < CAP - 1; ++t) {
            wv[t] = wv[t + 1];
            wc[t] = wc[t + 1];
        }
        --q;
    }
}

__global__ void __launch_bounds__(kB) patch_kernel(int npatch, const int *patch_node, const int *patch_variant, int n,
                                                   const int *Ap, const int *Aj, const double *Av, const int *rank,
                                                   double *patches, int *fill_idx, unsigned long long *status)
{
    const int j = blockIdx.x * kB + threadIdx.x;
    if (j >= npatch) return;
    const int c = patch_node[j];
    double *out = patches + (size_t)j * kPatch;
    int *idx = fill_idx + (size_t)j * kIdx;
    for (int t = 0; t < kPatch; ++t) out[t] = -1.0;
    for (int t = 0; t < kIdx; ++t) idx[t] = -1;
    if (c < 0 || c >= n) {
        refuse(status, j, LMG_NMG2D_COLUMN);
        return;
    }

    // row c: its diagonal and its positive neighbours in column order
    int where[7];
    double row[7];
    int k = 0;
    double d = 0.0;
    for (int e = Ap[c]; e < Ap[c + 1]; ++e) {
        const int col = Aj[e];
        const double v = Av[e];
        if (col == c) d = v;
        else if (v > 0.0) {
            if (k == 7) {
                refuse(status, j, LMG_NMG2D_VALENCE);
                return;
            }
            where[k] = col;
            row[k] = v;
            ++k;
        }
    }
    if (k == 7) {
        // the neighbours stably sorted by value: patch a leaves out the a-th smallest
        const int a = patch_variant[j];
        int drop = 0;
        for (int t = 0; t < 7; ++t) {
            int before = 0;
            for (int u = 0; u < 7; ++u) before += (row[u] < row[t] || (row[u] == row[t] && u < t)) ? 1 : 0;
            if (before == a) drop = t;
        }
        for (int t = drop; t < 6; ++t) {
            where[t] = where[t + 1];
            row[t] = row[t + 1];
        }
        k = 6;
    }
    if (k < 2) {
        refuse(status, j, LMG_NMG2D_FEW);
        return;
    }
    out[0] = d;
    for (int t = 0; t < 6; ++t) out[1 + t] = t < k ? row[t] : d / scale_down(k);
    idx[0] = c;
    for (int t = 0; t < k; ++t) idx[1 + t] = where[t];

    int second[6], nsecond = 0;
    for (int b = 0; b < k; ++b) {
        const int nb = where[b];
        double wv[6], g = 0.0;
        int wc[6], q = 0;
        for (int e = Ap[nb]; e < Ap[nb + 1]; ++e) {
            const int col = Aj[e];
            const double v = Av[e];
            if (col == c || v == 0.0) continue;
            if (rank[col] >= 0) {
                // a coarse second neighbour of c: first occurrences, in the order the rows show them
                bool known = false;
                for (int t = 0; t < k; ++t) known |= where[t] == col;
                for (int t = 0; t < nsecond; ++t) known |= second[t] == col;
                if (!known) {
                    if (nsecond == 6) {
                        refuse(status, j, LMG_NMG2D_SECOND);
                        return;
                    }
                    second[nsecond++] = col;
                }
            }
            if (col == nb) g = v;
            else if (v > 0.0) window_push<6>(wv, wc, q, v, col);
        }
        if (q == 0) {
            refuse(status, j, LMG_NMG2D_ISOLATED);
            return;
        }
        double *blk = out + 7 + 6 * b;
        blk[0] = g;
        for (int t = 0; t < 5; ++t) blk[1 + t] = t < q ? wv[t] : g / scale_down(q + 1);

        // the coarse nodes behind this neighbour's kept neighbours: first occurrences in order, the last three
        int cand[35], ncand = 0;
        for (int t = 0; t < q; ++t) {
            const int kk = wc[t];
            double xv[8];
            int xc[8], m = 0;
            for (int e = Ap[kk]; e < Ap[kk + 1]; ++e)
                if (Av[e] != 0.0) window_push<8>(xv, xc, m, Av[e], Aj[e]);
            for (int u = 0; u < m; ++u) {
                const int col = xc[u];
                if (col == c || rank[col] < 0) continue;
                bool known = false;
                for (int s = 0; s < ncand; ++s) known |= cand[s] == col;
                if (!known) cand[ncand++] = col;          // ncand <= 5 * 7
            }
        }
        const int first = ncand > 3 ? ncand - 3 : 0;
        for (int t = first; t < ncand; ++t) idx[13 + 3 * b + (t - first)] = cand[t];
    }
    for (int b = k; b < 6; ++b) {
        double *blk = out + 7 + 6 * b;
        blk[0] = d * scale_up(k);
        for (int t = 1; t < 6; ++t) blk[t] = d / scale_down(k);
    }
    for (int t = 0; t < nsecond; ++t) idx[7 + t] = second[t];
}

constexpr long long kNoKey = LLONG_MAX;

// slot t of patch j -> (row, col) of B or nothing: t = 0 (c, n_c); 1..6 (where[t-1], n_c); 7..12 (c, coarse(idx[t]));
// 13 + 3 b + u (where[b], coarse(idx[t]))
__global__ void __launch_bounds__(kB) contrib_kernel(long long total, int n, int nc, const int *fill_idx, const int *rank,
                                                     long long *keys, unsigned long long *status)
{
    const long long s = (long long)blockIdx.x * kB + threadIdx.x;
    if (s >= total) return;
    const long long j = s / kIdx;
    const int t = (int)(s - j * kIdx);
    const int *idx = fill_idx + j * kIdx;
    const int node = idx[t], c = idx[0];
    long long key = kNoKey;
    bool bad = c < 0 || c >= n || node >= n;
    if (!bad && node >= 0) {
        int r, col;
        if (t < 7) {
            r = node;
            col = rank[c];
        } else {
            r = t < 13 ? c : idx[1 + (t - 13) / 3];
            col = rank[node];
        }
        bad = r < 0 || r >= n || col < 0 || col >= nc;
        if (!bad) key = (long long)r * nc + col;
    }
    if (bad) refuse(status, j, LMG_NMG2D_COLUMN);
    keys[s] = key;
}

// entry e: the run [start[e], start[e+1]) of the stably sorted keys; slot[] is the sort's permutation (patch order inside
// a run).  cur = p if cur == 0 else (cur + p) / 2, from cur = 0.
__global__ void __launch_bounds__(kB) fold_kernel(long long nentries, const long long *start, const long long *keys,
                                                  const long long *slot, const double *res, int nc, int *row, int *col,
                                                  double *val)
{
    const long long e = (long long)blockIdx.x * kB + threadIdx.x;
    if (e >= nentries) return;
    double cur = 0.0;
    for (long long i = start[e]; i < start[e + 1]; ++i) {
        const double p = res[slot[i]];
        cur = cur == 0.0 ? p : (cur + p) / 2.0;
    }
    const long long key = keys[start[e]];
    row[e] = (int)(key / nc);
    col[e] = (int)(key % nc);
    val[e] = cur;
}

__global__ void __launch_bounds__(kB) normalize_kernel(int n, const int *Bp, const double *Bv, double *Qv)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    double sum = 0.0;
    for (int k = Bp[i]; k < Bp[i + 1]; ++k) sum += Bv[k];
    for (int k = Bp[i]; k < Bp[i + 1]; ++k) Qv[k] = Bv[k] / sum;
}

__global__ void __launch_bounds__(kB) dneighs_kernel(int nc, const int *last_patch, const int *fill_idx, const int *rank,
                                                     int *dn)
{
    const int r = blockIdx.x * kB + threadIdx.x;
    if (r >= nc) return;
    const int *idx = fill_idx + (size_t)last_patch[r] * kIdx;
    for (int t = 0; t < 6; ++t) dn[r * 6 + t] = idx[7 + t] >= 0 ? rank[idx[7 + t]] : -1;
}

__device__ __forceinline__ bool cut_keeps(const int *dn, int i, int j)
{
    bool keep = j == i;
    for (int t = 0; t < 6; ++t) keep |= dn[i * 6 + t] == j;
    return keep;
}

__global__ void __launch_bounds__(kB) cut_mark_kernel(int n, const int *Ap, const int *Aj, const int *dn, int *rownnz)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    int kept = 0;
    for (int k = Ap[i]; k < Ap[i + 1]; ++k) kept += cut_keeps(dn, i, Aj[k]) ? 1 : 0;
    rownnz[i] = kept;
}

__global__ void __launch_bounds__(kB) cut_fill_kernel(int n, const int *Ap, const int *Aj, const double *Av, const int *dn,
                                                      const int *Cp, int *Cj, double *Cv)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    int at = Cp[i];
    for (int k = Ap[i]; k < Ap[i + 1]; ++k)
        if (cut_keeps(dn, i, Aj[k])) {
            Cj[at] = Aj[k];
            Cv[at] = Av[k];
            ++at;
        }
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + kB - 1) / kB); }
inline bool rows_ok(int64_t n) { return n >= 0 && n < INT32_MAX - kB; }

}  // namespace

extern "C" {

int lmg_nmg2d_check(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, uint64_t *status,
                    void *stream)
{
    if (!rows_ok(n) || !rowptr || !status) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    check_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, rowptr, colidx, vals, (unsigned long long *)status);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_nmg2d_count(int64_t nc, const int32_t *coarse_nodes, const int32_t *rowptr, const int32_t *colidx, const double *vals,
                    int32_t *extra, uint64_t *status, void *stream)
{
    if (!rows_ok(nc) || !rowptr || !status || (nc > 0 && (!coarse_nodes || !extra))) return LMG_ERR_ARG;
    if (nc == 0) return LMG_OK;
    count_kernel<<<blocks(nc), kB, 0, lmg_stream(stream)>>>((int)nc, coarse_nodes, rowptr, colidx, vals, extra,
                                                           (unsigned long long *)status);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_nmg2d_patches(int64_t npatch, const int32_t *patch_node, const int32_t *patch_variant, int64_t n,
                      const int32_t *rowptr, const int32_t *colidx, const double *vals, const int32_t *rank, double *patches,
                      int32_t *fill_idx, uint64_t *status, void *stream)
{
    if (!rows_ok(npatch) || !rows_ok(n) || npatch * kPatch >= INT32_MAX || !rowptr || !rank || !status) return LMG_ERR_ARG;
    if (npatch == 0) return LMG_OK;
    if (!patch_node || !patch_variant || !patches || !fill_idx) return LMG_ERR_ARG;
    patch_kernel<<<blocks(npatch), kB, 0, lmg_stream(stream)>>>((int)npatch, patch_node, patch_variant, (int)n, rowptr, colidx,
                                                               vals, rank, patches, fill_idx, (unsigned long long *)status);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_nmg2d_contrib(int64_t npatch, int64_t n, int64_t nc, const int32_t *fill_idx, const int32_t *rank, int64_t *keys,
                      uint64_t *status, void *stream)
{
    if (!rows_ok(npatch) || !rows_ok(n) || !rows_ok(nc) || nc < 1 || npatch * kPatch >= INT32_MAX || !status) return LMG_ERR_ARG;
    if (npatch == 0) return LMG_OK;
    if (!fill_idx || !rank || !keys) return LMG_ERR_ARG;
    const int64_t total = npatch * kIdx;
    contrib_kernel<<<blocks(total), kB, 0, lmg_stream(stream)>>>((long long)total, (int)n, (int)nc, fill_idx, rank,
                                                                (long long *)keys, (unsigned long long *)status);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_nmg2d_fold(int64_t nentries, const int64_t *start, const int64_t *keys, const int64_t *slot, const double *res,
                   int64_t nc, int32_t *row, int32_t *col, double *val, void *stream)
{
    if (!rows_ok(nentries) || !rows_ok(nc) || nc < 1) return LMG_ERR_ARG;
    if (nentries == 0) return LMG_OK;
    if (!start || !keys || !slot || !res || !row || !col || !val) return LMG_ERR_ARG;
    fold_kernel<<<blocks(nentries), kB, 0, lmg_stream(stream)>>>((long long)nentries, (const long long *)start,
                                                                (const long long *)keys, (const long long *)slot, res, (int)nc,
                                                                row, col, val);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_nmg2d_normalize(int64_t n, const int32_t *rowptr, const double *b_vals, double *q_vals, void *stream)
{
    if (!rows_ok(n) || !rowptr) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    normalize_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, rowptr, b_vals, q_vals);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_nmg2d_dneighs(int64_t nc, const int32_t *last_patch, const int32_t *fill_idx, const int32_t *rank, int32_t *d_neighs,
                      void *stream)
{
    if (!rows_ok(nc) || nc * 6 >= INT32_MAX) return LMG_ERR_ARG;
    if (nc == 0) return LMG_OK;
    if (!last_patch || !fill_idx || !rank || !d_neighs) return LMG_ERR_ARG;
    dneighs_kernel<<<blocks(nc), kB, 0, lmg_stream(stream)>>>((int)nc, last_patch, fill_idx, rank, d_neighs);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_nmg2d_cut_mark(int64_t n, const int32_t *rowptr, const int32_t *colidx, const int32_t *d_neighs, int32_t *rownnz,
                       void *stream)
{
    if (!rows_ok(n) || n * 6 >= INT32_MAX || !rowptr) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!d_neighs || !rownnz) return LMG_ERR_ARG;
    cut_mark_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, rowptr, colidx, d_neighs, rownnz);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_nmg2d_cut_fill(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *vals, const int32_t *d_neighs,
                       const int32_t *cut_rowptr, int32_t *cut_colidx, double *cut_vals, void *stream)
{
    if (!rows_ok(n) || n * 6 >= INT32_MAX || !rowptr) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!d_neighs || !cut_rowptr) return LMG_ERR_ARG;
    cut_fill_kernel<<<blocks(n), kB, 0, lmg_stream(stream)>>>((int)n, rowptr, colidx, vals, d_neighs, cut_rowptr, cut_colidx,
                                                             cut_vals);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

}  // extern "C"
