// Triangle meshes on the device: the stage before assembly (learn_multigrid/mesh/Mesh2D.py: construct :63-93, refine
// :95-160; assembly.P1Mesh2D.__init__ for the mesh graph; thesis_structured_2d.py:407-414 for the identity rows).
//
// The reference refines with a loop over elements and edges that looks every edge up in an n x n lil_matrix and numbers
// a midpoint when it first meets the edge.  Here the same numbering is stated without the loop:
//   slot    s = 3 e + k is the directed edge conn[e][k] -> conn[e][(k + 1) % 3]; its key is min << 32 | max
//   run     after the caller's STABLE sort of the keys with their slots, the slots of one undirected edge are
//           neighbours, ascending; the first is the run's head.  One lane per run start walks its run and tells every
//           slot its head; a run of length 1 is a boundary edge, longer than 2 a non-manifold one (still one midpoint)
//   number  the loop meets the edges in the order of their head slots, so the midpoint of a run is
//           n + (heads before its head) -- the caller's exclusive scan of the head flags
//   write   the head slot's element stores the point r * p[left] + (1 - r) * p[right] (one writer); every element
//           writes its four children [t0 v1 t1] [t1 v2 t2] [t0 t1 t2] [v0 t0 t2]
// The mesh graph: node -> (element, local vertex) is the caller's stable sort of conn, split here; a pattern row is
// owned by one lane, which collects the vertices of the node's elements as a sorted set in LDS (count / caller's scan /
// fill, both passes with the same code), so nothing is added atomically and two calls give the same bits.
// A refusal -- an index outside the mesh, a repeated vertex, a masked row without a diagonal -- goes to one 64-bit
// status word as (order << 8 | rule) with an atomic minimum: the lowest offender is named whatever the arrival order.
#include "lmg_common.hpp"

namespace {

constexpr int kB = 256;
constexpr int kRowB = 64;           // pattern rows: one wave, kMaxCols * kRowB column slots in LDS (16 KiB)
constexpr int kMaxCols = 64;        // distinct columns per pattern row

__device__ __forceinline__ void refuse(unsigned long long *status, long long order, int rule)
{
    atomicMin(status, ((unsigned long long)order << 8) | (unsigned long long)rule);
}

// ---- structured mesh ------------------------------------------------------------------------------------------------
// node i = (row j, column c) of a (v_el + 1) x (h_el + 1) grid, h fastest; coordinate c * (1 / h_el), the last one 1.0:
// np.linspace(0, 1, h_el + 1).  Square q gives (k, k+1, k+W+1), (k, k+W+1, k+W), one after the other.
__global__ void __launch_bounds__(kB) construct_kernel(int h_el, int v_el, double *px, double *py, int *conn)
{
    const int W = h_el + 1, n = W * (v_el + 1), nsq = h_el * v_el;
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const int c = i % W, j = i / W;
    px[i] = c == h_el ? 1.0 : (double)c * (1.0 / (double)h_el);
    py[i] = j == v_el ? 1.0 : (double)j * (1.0 / (double)v_el);
    if (i >= nsq) return;
    const int k = (i / h_el) * W + i % h_el;
    int *o = conn + 6 * (size_t)i;
    o[0] = k, o[1] = k + 1, o[2] = k + W + 1;
    o[3] = k, o[4] = k + W + 1, o[5] = k + W;
}

__global__ void __launch_bounds__(kB) check_kernel(int n, int ne, const int *conn, unsigned long long *status)
{
    const int e = blockIdx.x * kB + threadIdx.x;
    if (e >= ne) return;
    const int a = conn[3 * (size_t)e], b = conn[3 * (size_t)e + 1], c = conn[3 * (size_t)e + 2];
    if (a < 0 || a >= n || b < 0 || b >= n || c < 0 || c >= n) refuse(status, e, LMG_MESH2D_INDEX);
    else if (a == b || b == c || a == c) refuse(status, e, LMG_MESH2D_REPEATED);
}

// ---- edges ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kB) edge_keys_kernel(int nslots, const int *conn, long long *keys)
{
    const int s = blockIdx.x * kB + threadIdx.x;
    if (s >= nslots) return;
    const int k = s % 3, e0 = s - k;
    const int l = conn[s], r = conn[e0 + (k == 2 ? 0 : k + 1)];
    keys[s] = ((long long)(unsigned)min(l, r) << 32) | (long long)(unsigned)max(l, r);
}

// one lane per sorted position; the lane at a run's start owns the run
__global__ void __launch_bounds__(kB) edge_runs_kernel(int nslots, const long long *keys, const long long *slot, int n,
                                                       int *head, int *is_head, unsigned char *mask)
{
    const int j = blockIdx.x * kB + threadIdx.x;
    if (j >= nslots) return;
    const long long key = keys[j], s = slot[j];
    if (s < 0 || s >= nslots) return;                       // (not a permutation: the caller's sort is broken)
    const bool start = j == 0 || keys[j - 1] != key;
    is_head[s] = start ? 1 : 0;
    if (!start) return;
    int len = 0;
    for (int k = j; k < nslots && keys[k] == key; ++k, ++len) {
        const long long t = slot[k];
        if (t >= 0 && t < nslots) head[t] = (int)s;
    }
    if (mask && len == 1) {
        const long long lo = key >> 32, hi = key & 0xFFFFFFFFll;
        // (several boundary edges meet in a node: all store the same 1)
        if (lo >= 0 && lo < n) mask[lo] = 1;
        if (hi >= 0 && hi < n) mask[hi] = 1;
    }
}

// ---- refinement -----------------------------------------------------------------------------------------------------
// lane i copies node i (i < n) and refines element i (i < ne)
__global__ void __launch_bounds__(kB) refine_kernel(int n, int ne, int edges, const double *px, const double *py,
                                                    const int *conn, const int *head, const int *rank,
                                                    const double *ratio, double *opx, double *opy, int *oconn)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i < n) {
        opx[i] = px[i];
        opy[i] = py[i];
    }
    if (i >= ne) return;
    const int s0 = 3 * i;
    const int v0 = conn[s0], v1 = conn[s0 + 1], v2 = conn[s0 + 2];
    int t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int h = head[s0 + k];
        const int r = (h >= 0 && h < 3 * ne) ? rank[h] : -1;
        t[k] = n + r;
        if (h != s0 + k || r < 0 || r >= edges) continue;   // the midpoint has another writer (or nowhere to go)
        const int left = k == 0 ? v0 : (k == 1 ? v1 : v2), right = k == 0 ? v1 : (k == 1 ? v2 : v0);
        if (left < 0 || left >= n || right < 0 || right >= n) continue;
        const double q = ratio ? ratio[r] : 0.5;
        opx[n + r] = q * px[left] + (1.0 - q) * px[right];
        opy[n + r] = q * py[left] + (1.0 - q) * py[right];
    }
    int *o = oconn + 12 * (size_t)i;
    o[0] = t[0], o[1] = v1, o[2] = t[1];
    o[3] = t[1], o[4] = v2, o[5] = t[2];
    o[6] = t[0], o[7] = t[1], o[8] = t[2];
    o[9] = v0, o[10] = t[0], o[11] = t[2];
}

// ---- the mesh graph -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kB) n2e_kernel(int nslots, const long long *order, int *elem, int *loc)
{
    const int j = blockIdx.x * kB + threadIdx.x;
    if (j >= nslots) return;
    const long long s = order[j];
    elem[j] = (int)(s / 3);
    loc[j] = (int)(s % 3);
}

// c into the ascending list cols[0], cols[kRowB], ... (len entries); len = kMaxCols + 1 if it does not fit
__device__ __forceinline__ void set_insert(int *cols, int &len, int c)
{
    int p = 0;
    while (p < len && cols[p * kRowB] < c) ++p;
    if (p < len && cols[p * kRowB] == c) return;
    if (len >= kMaxCols) {
        len = kMaxCols + 1;
        return;
    }
    for (int j = len; j > p; --j) cols[j * kRowB] = cols[(j - 1) * kRowB];
    cols[p * kRowB] = c;
    ++len;
}

template <bool FILL>
__global__ void __launch_bounds__(kRowB) rows_kernel(int n, int ne, const int *conn, const int *n2e_ptr,
                                                     const int *n2e_elem, const int *rowptr, int nnz, int *out)
{
    __shared__ int s_cols[kMaxCols * kRowB];             // slot k of lane t at k * kRowB + t: no bank conflicts
    const int i = blockIdx.x * kRowB + threadIdx.x;
    if (i >= n) return;
    int *cols = s_cols + threadIdx.x;
    int len = 0;
    const int k0 = max(n2e_ptr[i], 0), k1 = min(n2e_ptr[i + 1], 3 * ne);
    for (int k = k0; k < k1 && len <= kMaxCols; ++k) {
        const int e = n2e_elem[k];
        if (e < 0 || e >= ne) continue;
        set_insert(cols, len, conn[3 * e]);
        if (len <= kMaxCols) set_insert(cols, len, conn[3 * e + 1]);
        if (len <= kMaxCols) set_insert(cols, len, conn[3 * e + 2]);
    }
    if (!FILL) {
        out[i] = len;
        return;
    }
    const int s = rowptr[i];
    if (len > kMaxCols || s < 0 || rowptr[i + 1] - s != len || s + len > nnz) return;   // (not the counted row)
    for (int j = 0; j < len; ++j) out[s + j] = cols[j * kRowB];
}

// ---- identity rows --------------------------------------------------------------------------------------------------
// APPLY false: every masked row must store its diagonal.  APPLY true (the next launch): nothing if a row was refused.
template <bool APPLY>
__global__ void __launch_bounds__(kB) identity_rows_kernel(int n, const int *rowptr, const int *colidx, double *vals,
                                                           const unsigned char *mask, const double *value, double *rhs,
                                                           unsigned long long *status)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n || !mask[i]) return;
    if (APPLY && *status != ~0ull) return;
    int d = -1;
    for (int k = rowptr[i]; k < rowptr[i + 1]; ++k)
        if (colidx[k] == i) {
            d = k;
            break;
        }
    if (!APPLY) {
        if (d < 0) refuse(status, i, LMG_MESH2D_DIAGONAL);
        return;
    }
    for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) vals[k] = k == d ? 1.0 : 0.0;
    if (rhs) rhs[i] = value ? value[i] : 0.0;
}

unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
// sizes every kernel of this file indexes with int: nodes, slots (3 per element)
bool sizes_ok(int64_t n, int64_t ne) { return n >= 1 && n < INT32_MAX && ne >= 1 && 3 * ne < INT32_MAX; }

}  // namespace

extern "C" {

int lmg_mesh2d_limits(int32_t *max_columns)
{
    if (!max_columns) return LMG_ERR_ARG;
    *max_columns = kMaxCols;
    return LMG_OK;
}

int lmg_mesh2d_construct(int64_t h_el, int64_t v_el, double *d_px, double *d_py, int32_t *d_conn, void *stream)
{
    if (h_el < 1 || v_el < 1 || h_el >= INT32_MAX || v_el >= INT32_MAX || !d_px || !d_py || !d_conn) return LMG_ERR_ARG;
    const int64_t n = (h_el + 1) * (v_el + 1);              // (both factors < 2^31: no overflow)
    if (!sizes_ok(n, 2 * h_el * v_el)) return LMG_ERR_ARG;
    construct_kernel<<<blocks(n, kB), kB, 0, lmg_stream(stream)>>>((int)h_el, (int)v_el, d_px, d_py, d_conn);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_mesh2d_check(int64_t n, int64_t ne, const int32_t *d_conn, uint64_t *d_status, void *stream)
{
    if (!sizes_ok(n, ne) || !d_conn || !d_status) return LMG_ERR_ARG;
    check_kernel<<<blocks(ne, kB), kB, 0, lmg_stream(stream)>>>((int)n, (int)ne, d_conn, (unsigned long long *)d_status);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_mesh2d_edge_keys(int64_t ne, const int32_t *d_conn, int64_t *d_keys, void *stream)
{
    if (!sizes_ok(1, ne) || !d_conn || !d_keys) return LMG_ERR_ARG;
    edge_keys_kernel<<<blocks(3 * ne, kB), kB, 0, lmg_stream(stream)>>>((int)(3 * ne), d_conn, (long long *)d_keys);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_mesh2d_edge_runs(int64_t n, int64_t ne, const int64_t *d_keys, const int64_t *d_slot, int32_t *d_head,
                         int32_t *d_is_head, uint8_t *d_mask, void *stream)
{
    if (!sizes_ok(n, ne) || !d_keys || !d_slot || !d_head || !d_is_head) return LMG_ERR_ARG;
    edge_runs_kernel<<<blocks(3 * ne, kB), kB, 0, lmg_stream(stream)>>>((int)(3 * ne), (const long long *)d_keys,
                                                                        (const long long *)d_slot, (int)n, d_head, d_is_head,
                                                                        d_mask);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_mesh2d_refine(int64_t n, int64_t ne, int64_t edges, const double *d_px, const double *d_py, const int32_t *d_conn,
                      const int32_t *d_head, const int32_t *d_rank, const double *d_ratio, double *d_px_out,
                      double *d_py_out, int32_t *d_conn_out, void *stream)
{
    if (!sizes_ok(n, ne) || edges < 1 || edges > 3 * ne || n + edges >= INT32_MAX) return LMG_ERR_ARG;
    if (!d_px || !d_py || !d_conn || !d_head || !d_rank || !d_px_out || !d_py_out || !d_conn_out) return LMG_ERR_ARG;
    if (d_px_out == d_px || d_py_out == d_py || d_conn_out == d_conn) return LMG_ERR_ARG;
    refine_kernel<<<blocks(n > ne ? n : ne, kB), kB, 0, lmg_stream(stream)>>>((int)n, (int)ne, (int)edges, d_px, d_py, d_conn,
                                                                              d_head, d_rank, d_ratio, d_px_out, d_py_out,
                                                                              d_conn_out);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_mesh2d_n2e_fill(int64_t ne, const int64_t *d_order, int32_t *d_elem, int32_t *d_loc, void *stream)
{
    if (!sizes_ok(1, ne) || !d_order || !d_elem || !d_loc) return LMG_ERR_ARG;
    n2e_kernel<<<blocks(3 * ne, kB), kB, 0, lmg_stream(stream)>>>((int)(3 * ne), (const long long *)d_order, d_elem, d_loc);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_mesh2d_rows_count(int64_t n, int64_t ne, const int32_t *d_conn, const int32_t *d_n2e_ptr,
                          const int32_t *d_n2e_elem, int32_t *d_rownnz, void *stream)
{
    if (!sizes_ok(n, ne) || !d_conn || !d_n2e_ptr || !d_n2e_elem || !d_rownnz) return LMG_ERR_ARG;
    rows_kernel<false><<<blocks(n, kRowB), kRowB, 0, lmg_stream(stream)>>>((int)n, (int)ne, d_conn, d_n2e_ptr, d_n2e_elem,
                                                                           nullptr, 0, d_rownnz);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_mesh2d_rows_fill(int64_t n, int64_t ne, const int32_t *d_conn, const int32_t *d_n2e_ptr,
                         const int32_t *d_n2e_elem, int64_t nnz, int32_t max_row, const int32_t *d_rowptr,
                         int32_t *d_colidx, void *stream)
{
    if (!sizes_ok(n, ne) || !d_conn || !d_n2e_ptr || !d_n2e_elem || !d_rowptr) return LMG_ERR_ARG;
    if (nnz < 0 || nnz >= INT32_MAX || max_row < 0 || (nnz > 0 && !d_colidx)) return LMG_ERR_ARG;
    if (max_row > kMaxCols) return LMG_ERR_CAPACITY;
    rows_kernel<true><<<blocks(n, kRowB), kRowB, 0, lmg_stream(stream)>>>((int)n, (int)ne, d_conn, d_n2e_ptr, d_n2e_elem,
                                                                          d_rowptr, (int)nnz, d_colidx);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_csr_identity_rows(int64_t n, const int32_t *d_rowptr, const int32_t *d_colidx, double *d_vals,
                          const uint8_t *d_mask, const double *d_value, double *d_rhs, uint64_t *d_status, void *stream)
{
    if (n < 0 || n >= INT32_MAX || !d_rowptr || !d_mask || !d_status) return LMG_ERR_ARG;
    if (n == 0) return LMG_OK;
    if (!d_colidx || !d_vals) return LMG_ERR_ARG;
    unsigned long long *st = (unsigned long long *)d_status;
    identity_rows_kernel<false><<<blocks(n, kB), kB, 0, lmg_stream(stream)>>>((int)n, d_rowptr, d_colidx, d_vals, d_mask,
                                                                              d_value, d_rhs, st);
    LMG_CHECK_LAUNCH();
    identity_rows_kernel<true><<<blocks(n, kB), kB, 0, lmg_stream(stream)>>>((int)n, d_rowptr, d_colidx, d_vals, d_mask,
                                                                             d_value, d_rhs, st);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

}  // extern "C"
