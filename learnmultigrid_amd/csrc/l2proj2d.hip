// 2-D L2-projection coupling operator between two P1 triangle meshes that need not be nested.
//
// The reference stops at a stub here (L2Projection.compute_transfer_2d; Intersection.find_intersections2d assumes four
// children per coarse element), so the rules are this project's own; l2_projection.coupling_operator_2d states them on
// the host and this file follows them:
//   pairs   (fine element e, coarse element c) whose bounding boxes overlap, found through a uniform cell grid over the
//           coarse mesh: work proportional to the pairs, never ne_f * ne_c
//   clip    e against the three edges of c by Sutherland-Hodgman, c taken counter-clockwise, inside = side >= 0, a
//           crossing = P + (Q - P) * s_P / (s_P - s_Q); at most kPoly vertices
//   drop    the polygon's area (fan from vertex 0, |det| / 2 each) must exceed area_tol * min(|T_e|, |T_c|)
//   rule    three points (1/6, 1/6), (1/6, 2/3), (2/3, 1/6), weight |det| / 6 each, on every fan triangle with det != 0
//
// Search: every coarse element is entered into the cells its box overlaps (count / caller's scan / fill as 64-bit keys
// cell << 32 | element, which the caller sorts); every fine element then walks the cells of its own box and keeps an
// entry in the first cell the two cell ranges share -- no duplicates without a set -- if the boxes themselves overlap
// (count / scan / fill, each list ascending).
// Rows: one lane owns one fine node, walks its elements in ascending order and each element's candidates in ascending
// order, and recomputes the clip of every pair: nothing per pair is stored, nothing is added atomically.  A counting
// pass finds the distinct coarse nodes of the row, the filling pass builds the row in place, columns ascending.  Both
// decide every pair with the same code (row_walk).
#include "lmg_common.hpp"

namespace {

constexpr int kB = 256;             // search kernels
constexpr int kRowB = 64;           // row kernels: one wave, kMaxCols * kRowB column slots in LDS for the counting pass
constexpr int kPoly = 7;            // vertices a clipped polygon holds (l2_projection.POLY)
constexpr int kMaxCand = 64;        // candidates per fine element
constexpr int kMaxCols = 64;        // distinct columns per row
constexpr int kMaxCells = 46340;    // cells per direction: their square fits int32

struct Mesh {
    const double *px, *py;
    const int *conn;
};
struct Tri {
    double x0, y0, x1, y1, x2, y2;
};
struct Grid {                       // d_grid: origin, far corner, cells per unit length
    double ox, oy, ex, ey, ix, iy;
    int nc;
};
struct Box {
    double xlo, xhi, ylo, yhi;
};

__device__ __forceinline__ Tri load_tri(const Mesh &m, int e)
{
    const int a = m.conn[3 * e], b = m.conn[3 * e + 1], c = m.conn[3 * e + 2];
    return {m.px[a], m.py[a], m.px[b], m.py[b], m.px[c], m.py[c]};
}
__device__ __forceinline__ double det3(double ax, double ay, double bx, double by, double cx, double cy)
{
    return (bx - ax) * (cy - ay) - (cx - ax) * (by - ay);
}
__device__ __forceinline__ Box box_of(const Tri &t)
{
    return {fmin(t.x0, fmin(t.x1, t.x2)), fmax(t.x0, fmax(t.x1, t.x2)), fmin(t.y0, fmin(t.y1, t.y2)),
            fmax(t.y0, fmax(t.y1, t.y2))};
}
__device__ __forceinline__ Grid load_grid(const double *g, int nc)
{
    return {g[0], g[1], g[2], g[3], g[4], g[5], nc};
}
// monotone in v, so overlapping boxes have overlapping cell ranges
__device__ __forceinline__ int cell_of(double v, double org, double inv, int nc)
{
    const double f = floor((v - org) * inv);
    return f > 0.0 ? (f < (double)(nc - 1) ? (int)f : nc - 1) : 0;
}
struct Cells {
    int x0, x1, y0, y1;
};
__device__ __forceinline__ Cells cells_of(const Box &b, const Grid &g)
{
    return {cell_of(b.xlo, g.ox, g.ix, g.nc), cell_of(b.xhi, g.ox, g.ix, g.nc), cell_of(b.ylo, g.oy, g.iy, g.nc),
            cell_of(b.yhi, g.oy, g.iy, g.nc)};
}

// ---- search -----------------------------------------------------------------------------------------------------------
template <bool FILL>
__global__ void __launch_bounds__(kB) cell_kernel(int ne_c, Mesh c, const double *d_grid, int nc, const int *ptr, int *cnt,
                                                  long long *keys, int total)
{
    const int e = blockIdx.x * kB + threadIdx.x;
    if (e >= ne_c) return;
    const Grid g = load_grid(d_grid, nc);
    const Cells r = cells_of(box_of(load_tri(c, e)), g);
    if (!FILL) {
        cnt[e] = (r.x1 - r.x0 + 1) * (r.y1 - r.y0 + 1);
        return;
    }
    int at = ptr[e];
    for (int y = r.y0; y <= r.y1; ++y)
        for (int x = r.x0; x <= r.x1; ++x, ++at)
            if (at < total) keys[at] = ((long long)(y * nc + x) << 32) | (long long)e;
}

template <bool FILL>
__global__ void __launch_bounds__(kB) cand_kernel(int ne_f, Mesh f, int ne_c, Mesh c, const double *d_grid, int nc,
                                                  const int *cellptr, const int *cellent, const int *candptr, int *out)
{
    const int e = blockIdx.x * kB + threadIdx.x;
    if (e >= ne_f) return;
    const Grid g = load_grid(d_grid, nc);
    const Box fb = box_of(load_tri(f, e));
    int n = 0;
    const int base = FILL ? candptr[e] : 0, room = FILL ? candptr[e + 1] - base : 0;
    if (fb.xhi >= g.ox && fb.xlo <= g.ex && fb.yhi >= g.oy && fb.ylo <= g.ey) {
        const Cells fr = cells_of(fb, g);
        for (int y = fr.y0; y <= fr.y1; ++y)
            for (int x = fr.x0; x <= fr.x1; ++x) {
                const int cell = y * nc + x;
                for (int k = cellptr[cell]; k < cellptr[cell + 1]; ++k) {
                    const int ce = cellent[k];
                    if (ce < 0 || ce >= ne_c) continue;
                    const Box cb = box_of(load_tri(c, ce));
                    const Cells cr = cells_of(cb, g);
                    // met in several cells: counts in the first cell the two ranges share
                    if (x != max(fr.x0, cr.x0) || y != max(fr.y0, cr.y0)) continue;
                    if (!(fb.xlo <= cb.xhi && cb.xlo <= fb.xhi && fb.ylo <= cb.yhi && cb.ylo <= fb.yhi)) continue;
                    if (FILL) {
                        if (n >= room) continue;                       // (the counting pass decided the same pairs)
                        int j = n;
                        for (; j > 0 && out[base + j - 1] > ce; --j) out[base + j] = out[base + j - 1];
                        out[base + j] = ce;
                    }
                    ++n;
                }
            }
    }
    if (!FILL) out[e] = n;
}

// ---- clipping: polygons in registers ---------------------------------------------------------------------------------
// Every index into x[] / y[] is a compile-time constant after unrolling, so the arrays live in VGPRs; a vertex is
// appended by comparing the running count with each slot.
struct Poly {
    double x[kPoly], y[kPoly];
    int n;
};
__device__ __forceinline__ void emit(Poly &o, double x, double y)
{
#pragma unroll
    for (int k = 0; k < kPoly; ++k)
        if (o.n == k) {
            o.x[k] = x;
            o.y[k] = y;
        }
    o.n += o.n < kPoly ? 1 : 0;
}
// `in` holds at most NIN vertices; out = in clipped to the left of a -> b
template <int NIN>
__device__ __forceinline__ void clip_edge(const Poly &in, Poly &out, double ax, double ay, double bx, double by)
{
    double s[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) s[i] = (bx - ax) * (in.y[i] - ay) - (by - ay) * (in.x[i] - ax);
    double px = in.x[0], py = in.y[0], ps = s[0];        // the vertex before vertex 0 is the last one
#pragma unroll
    for (int i = 1; i < NIN; ++i)
        if (in.n - 1 == i) {
            px = in.x[i];
            py = in.y[i];
            ps = s[i];
        }
    out.n = 0;
#pragma unroll
    for (int k = 0; k < kPoly; ++k) out.x[k] = out.y[k] = 0.0;
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        const double qx = in.x[i], qy = in.y[i], qs = s[i];
        const bool act = i < in.n, inq = qs >= 0.0, inp = ps >= 0.0;
        if (act && inq != inp) {
            const double t = ps / (ps - qs);
            emit(out, px + (qx - px) * t, py + (qy - py) * t);
        }
        if (act && inq) emit(out, qx, qy);
        px = qx;
        py = qy;
        ps = qs;
    }
}

// the intersection of F with C, or false if the drop rule removes the pair
__device__ __forceinline__ bool clip_pair(const Tri &F, const Tri &C, double det_f, double det_c, double area_tol, Poly &out)
{
    const bool cw = det_c < 0.0;
    const double c1x = cw ? C.x2 : C.x1, c1y = cw ? C.y2 : C.y1, c2x = cw ? C.x1 : C.x2, c2y = cw ? C.y1 : C.y2;
    Poly a, b;
    a.n = 3;
    a.x[0] = F.x0, a.y[0] = F.y0, a.x[1] = F.x1, a.y[1] = F.y1, a.x[2] = F.x2, a.y[2] = F.y2;
#pragma unroll
    for (int k = 3; k < kPoly; ++k) a.x[k] = a.y[k] = 0.0;
    clip_edge<3>(a, b, C.x0, C.y0, c1x, c1y);            // 3 vertices, two crossings at most: 4
    clip_edge<4>(b, a, c1x, c1y, c2x, c2y);              // 4 vertices, four crossings at most: 6
    clip_edge<6>(a, out, c2x, c2y, C.x0, C.y0);          // held to kPoly
    double area = 0.0;
#pragma unroll
    for (int t = 1; t < kPoly - 1; ++t) {
        const double d = t + 1 < out.n ? det3(out.x[0], out.y[0], out.x[t], out.y[t], out.x[t + 1], out.y[t + 1]) : 0.0;
        area += fabs(d) / 2.0;
    }
    return area > area_tol * fmin(fabs(det_f), fabs(det_c)) / 2.0;
}

// a0..a2 += integral over the polygon of (basis `ln` of F) x (the three bases of C)
__device__ __forceinline__ void integrate(const Poly &p, const Tri &F, const Tri &C, double det_f, double det_c, int ln,
                                          double &a0, double &a1, double &a2)
{
    const double xi[3] = {1.0 / 6.0, 1.0 / 6.0, 2.0 / 3.0}, eta[3] = {1.0 / 6.0, 2.0 / 3.0, 1.0 / 6.0};
    const double vx = p.x[0], vy = p.y[0];
#pragma unroll
    for (int t = 1; t < kPoly - 1; ++t) {
        const double d = t + 1 < p.n ? det3(vx, vy, p.x[t], p.y[t], p.x[t + 1], p.y[t + 1]) : 0.0;
        if (d == 0.0) continue;
        const double w = fabs(d) / 6.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double x = vx + (p.x[t] - vx) * xi[q] + (p.x[t + 1] - vx) * eta[q];
            const double y = vy + (p.y[t] - vy) * xi[q] + (p.y[t + 1] - vy) * eta[q];
            const double f0 = det3(x, y, F.x1, F.y1, F.x2, F.y2), f1 = det3(F.x0, F.y0, x, y, F.x2, F.y2),
                         f2 = det3(F.x0, F.y0, F.x1, F.y1, x, y);
            const double lf = (ln == 0 ? f0 : (ln == 1 ? f1 : f2)) / det_f;
            const double wl = w * lf;
            a0 += wl * (det3(x, y, C.x1, C.y1, C.x2, C.y2) / det_c);
            a1 += wl * (det3(C.x0, C.y0, x, y, C.x2, C.y2) / det_c);
            a2 += wl * (det3(C.x0, C.y0, C.x1, C.y1, x, y) / det_c);
        }
    }
}

// ---- rows -------------------------------------------------------------------------------------------------------------
// position of column c in the ascending list cols[0], cols[stride], ... (len entries, room for cap), inserted with a
// zero value if new; -1 and len = cap + 1 if it does not fit
template <bool FILL>
__device__ __forceinline__ int find_or_insert(int *cols, int stride, double *vals, int &len, int cap, int c)
{
    int p = 0;
    while (p < len && cols[p * stride] < c) ++p;
    if (p < len && cols[p * stride] == c) return p;
    if (len >= cap) {
        len = cap + 1;
        return -1;
    }
    for (int j = len; j > p; --j) {
        cols[j * stride] = cols[(j - 1) * stride];
        if (FILL) vals[j] = vals[j - 1];
    }
    cols[p * stride] = c;
    if (FILL) vals[p] = 0.0;
    ++len;
    return p;
}

struct RowArgs {
    int nf, ne_f, ncn, ne_c;
    Mesh f;
    const int *n2e_ptr, *n2e_elem, *n2e_loc;
    Mesh c;
    const int *candptr, *cand;
    double area_tol;
};

// The row of fine node i.  Returns the number of distinct columns, cap + 1 if there are more; FILL: vals[] holds B_i.
template <bool FILL>
__device__ __forceinline__ int row_walk(const RowArgs &a, int i, int *cols, int stride, double *vals, int cap, double &lumped)
{
    int len = 0;
    lumped = 0.0;
    for (int k = a.n2e_ptr[i]; k < a.n2e_ptr[i + 1]; ++k) {
        const int e = a.n2e_elem[k], ln = a.n2e_loc[k];
        if (e < 0 || e >= a.ne_f) continue;
        const Tri F = load_tri(a.f, e);
        const double det_f = det3(F.x0, F.y0, F.x1, F.y1, F.x2, F.y2);
        lumped += fabs(det_f) / 6.0;
        for (int q = a.candptr[e]; q < a.candptr[e + 1]; ++q) {
            const int ce = a.cand[q];
            if (ce < 0 || ce >= a.ne_c) continue;
            const Tri C = load_tri(a.c, ce);
            const double det_c = det3(C.x0, C.y0, C.x1, C.y1, C.x2, C.y2);
            Poly poly;
            if (!clip_pair(F, C, det_f, det_c, a.area_tol, poly)) continue;
            const int c0 = a.c.conn[3 * ce], c1 = a.c.conn[3 * ce + 1], c2 = a.c.conn[3 * ce + 2];
            find_or_insert<FILL>(cols, stride, vals, len, cap, c0);
            find_or_insert<FILL>(cols, stride, vals, len, cap, c1);
            find_or_insert<FILL>(cols, stride, vals, len, cap, c2);
            if (len > cap) return len;
            if (FILL) {
                // (an insertion moves what lies above it: look the three up once all are in)
                const int p0 = find_or_insert<FILL>(cols, stride, vals, len, cap, c0);
                const int p1 = find_or_insert<FILL>(cols, stride, vals, len, cap, c1);
                const int p2 = find_or_insert<FILL>(cols, stride, vals, len, cap, c2);
                double a0 = vals[p0], a1 = vals[p1], a2 = vals[p2];
                integrate(poly, F, C, det_f, det_c, ln, a0, a1, a2);
                vals[p0] = a0;
                vals[p1] = a1;
                vals[p2] = a2;
            }
        }
    }
    return len;
}

__global__ void __launch_bounds__(kRowB) rows_count_kernel(RowArgs a, int *rownnz)
{
    __shared__ int s_cols[kMaxCols * kRowB];             // slot k of lane t at k * kRowB + t: no bank conflicts
    const int i = blockIdx.x * kRowB + threadIdx.x;
    if (i >= a.nf) return;
    double lumped;
    rownnz[i] = row_walk<false>(a, i, s_cols + threadIdx.x, kRowB, nullptr, kMaxCols, lumped);
}

// kind 0: B, 1: "pseudo" (B / lumped fine mass), 2: "quasi" (B / row sum)
__global__ void __launch_bounds__(kRowB) rows_fill_kernel(RowArgs a, int kind, const int *rowptr, int nnz, int *colidx,
                                                          double *vals)
{
    const int i = blockIdx.x * kRowB + threadIdx.x;
    if (i >= a.nf) return;
    const int s = rowptr[i], cap = rowptr[i + 1] - s;
    if (cap <= 0 || s < 0 || s + cap > nnz) return;       // an empty row stays empty for every kind
    double lumped;
    double *v = vals + s;
    const int len = row_walk<true>(a, i, colidx + s, 1, v, cap, lumped);
    if (kind == 1) {
        for (int j = 0; j < len && j < cap; ++j) v[j] = v[j] / lumped;
    } else if (kind == 2) {
        double rs = 0.0;
        for (int j = 0; j < len && j < cap; ++j) rs += v[j];
        for (int j = 0; j < len && j < cap; ++j) v[j] = v[j] / rs;
    }
}

bool mesh_ok(int64_t ne, const double *px, const double *py, const int32_t *conn)
{
    return ne >= 1 && ne < INT32_MAX && px && py && conn;
}
unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

int lmg_l2p2d_limits(int32_t *max_candidates, int32_t *max_columns)
{
    if (!max_candidates || !max_columns) return LMG_ERR_ARG;
    *max_candidates = kMaxCand;
    *max_columns = kMaxCols;
    return LMG_OK;
}

int lmg_l2p2d_cell_count(int64_t ne_c, const double *d_cpx, const double *d_cpy, const int32_t *d_cconn,
                         const double *d_grid, int32_t ncell, int32_t *d_count, void *stream)
{
    if (!mesh_ok(ne_c, d_cpx, d_cpy, d_cconn) || !d_grid || ncell < 1 || ncell > kMaxCells || !d_count) return LMG_ERR_ARG;
    cell_kernel<false><<<blocks(ne_c, kB), kB, 0, lmg_stream(stream)>>>((int)ne_c, Mesh{d_cpx, d_cpy, d_cconn}, d_grid, ncell,
                                                                        nullptr, d_count, nullptr, 0);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_l2p2d_cell_fill(int64_t ne_c, const double *d_cpx, const double *d_cpy, const int32_t *d_cconn,
                        const double *d_grid, int32_t ncell, int64_t total, const int32_t *d_ptr, int64_t *d_keys,
                        void *stream)
{
    if (!mesh_ok(ne_c, d_cpx, d_cpy, d_cconn) || !d_grid || ncell < 1 || ncell > kMaxCells) return LMG_ERR_ARG;
    if (total < 0 || total >= INT32_MAX || !d_ptr || (total > 0 && !d_keys)) return LMG_ERR_ARG;
    cell_kernel<true><<<blocks(ne_c, kB), kB, 0, lmg_stream(stream)>>>((int)ne_c, Mesh{d_cpx, d_cpy, d_cconn}, d_grid, ncell,
                                                                       d_ptr, nullptr, (long long *)d_keys, (int)total);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_l2p2d_cand_count(int64_t ne_f, const double *d_fpx, const double *d_fpy, const int32_t *d_fconn, int64_t ne_c,
                         const double *d_cpx, const double *d_cpy, const int32_t *d_cconn, const double *d_grid,
                         int32_t ncell, const int32_t *d_cellptr, const int32_t *d_cellent, int32_t *d_count, void *stream)
{
    if (!mesh_ok(ne_f, d_fpx, d_fpy, d_fconn) || !mesh_ok(ne_c, d_cpx, d_cpy, d_cconn)) return LMG_ERR_ARG;
    if (!d_grid || ncell < 1 || ncell > kMaxCells || !d_cellptr || !d_cellent || !d_count) return LMG_ERR_ARG;
    cand_kernel<false><<<blocks(ne_f, kB), kB, 0, lmg_stream(stream)>>>((int)ne_f, Mesh{d_fpx, d_fpy, d_fconn}, (int)ne_c,
                                                                        Mesh{d_cpx, d_cpy, d_cconn}, d_grid, ncell, d_cellptr,
                                                                        d_cellent, nullptr, d_count);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_l2p2d_cand_fill(int64_t ne_f, const double *d_fpx, const double *d_fpy, const int32_t *d_fconn, int64_t ne_c,
                        const double *d_cpx, const double *d_cpy, const int32_t *d_cconn, const double *d_grid,
                        int32_t ncell, const int32_t *d_cellptr, const int32_t *d_cellent, int64_t pairs,
                        int32_t max_count, const int32_t *d_candptr, int32_t *d_cand, void *stream)
{
    if (!mesh_ok(ne_f, d_fpx, d_fpy, d_fconn) || !mesh_ok(ne_c, d_cpx, d_cpy, d_cconn)) return LMG_ERR_ARG;
    if (!d_grid || ncell < 1 || ncell > kMaxCells || !d_cellptr || !d_cellent || !d_candptr) return LMG_ERR_ARG;
    if (pairs < 0 || pairs >= INT32_MAX || max_count < 0 || (pairs > 0 && !d_cand)) return LMG_ERR_ARG;
    if (max_count > kMaxCand) return LMG_ERR_CAPACITY;
    cand_kernel<true><<<blocks(ne_f, kB), kB, 0, lmg_stream(stream)>>>((int)ne_f, Mesh{d_fpx, d_fpy, d_fconn}, (int)ne_c,
                                                                       Mesh{d_cpx, d_cpy, d_cconn}, d_grid, ncell, d_cellptr,
                                                                       d_cellent, d_candptr, d_cand);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

static int row_args(RowArgs &a, int64_t nf, int64_t ne_f, const double *d_fpx, const double *d_fpy, const int32_t *d_fconn,
                    const int32_t *d_n2e_ptr, const int32_t *d_n2e_elem, const int32_t *d_n2e_loc, int64_t nc, int64_t ne_c,
                    const double *d_cpx, const double *d_cpy, const int32_t *d_cconn, const int32_t *d_candptr,
                    const int32_t *d_cand, double area_tol)
{
    if (nf < 1 || nf >= INT32_MAX || nc < 1 || nc >= INT32_MAX) return LMG_ERR_ARG;
    if (!mesh_ok(ne_f, d_fpx, d_fpy, d_fconn) || !mesh_ok(ne_c, d_cpx, d_cpy, d_cconn)) return LMG_ERR_ARG;
    // (d_cand may be null: meshes that meet nowhere have no pairs)
    if (!d_n2e_ptr || !d_n2e_elem || !d_n2e_loc || !d_candptr || !(area_tol == area_tol)) return LMG_ERR_ARG;
    a = RowArgs{(int)nf, (int)ne_f, (int)nc, (int)ne_c, Mesh{d_fpx, d_fpy, d_fconn}, d_n2e_ptr, d_n2e_elem, d_n2e_loc,
                Mesh{d_cpx, d_cpy, d_cconn}, d_candptr, d_cand, area_tol};
    return LMG_OK;
}

int lmg_l2p2d_rows_count(int64_t nf, int64_t ne_f, const double *d_fpx, const double *d_fpy, const int32_t *d_fconn,
                         const int32_t *d_n2e_ptr, const int32_t *d_n2e_elem, const int32_t *d_n2e_loc, int64_t nc,
                         int64_t ne_c, const double *d_cpx, const double *d_cpy, const int32_t *d_cconn,
                         const int32_t *d_candptr, const int32_t *d_cand, double area_tol, int32_t *d_rownnz, void *stream)
{
    RowArgs a;
    const int rc = row_args(a, nf, ne_f, d_fpx, d_fpy, d_fconn, d_n2e_ptr, d_n2e_elem, d_n2e_loc, nc, ne_c, d_cpx, d_cpy,
                            d_cconn, d_candptr, d_cand, area_tol);
    if (rc != LMG_OK || !d_rownnz) return rc != LMG_OK ? rc : LMG_ERR_ARG;
    rows_count_kernel<<<blocks(nf, kRowB), kRowB, 0, lmg_stream(stream)>>>(a, d_rownnz);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

int lmg_l2p2d_rows_fill(int kind, int64_t nf, int64_t ne_f, const double *d_fpx, const double *d_fpy,
                        const int32_t *d_fconn, const int32_t *d_n2e_ptr, const int32_t *d_n2e_elem,
                        const int32_t *d_n2e_loc, int64_t nc, int64_t ne_c, const double *d_cpx, const double *d_cpy,
                        const int32_t *d_cconn, const int32_t *d_candptr, const int32_t *d_cand, double area_tol, int64_t nnz,
                        int32_t max_row, const int32_t *d_rowptr, int32_t *d_colidx, double *d_vals, void *stream)
{
    RowArgs a;
    const int rc = row_args(a, nf, ne_f, d_fpx, d_fpy, d_fconn, d_n2e_ptr, d_n2e_elem, d_n2e_loc, nc, ne_c, d_cpx, d_cpy,
                            d_cconn, d_candptr, d_cand, area_tol);
    if (rc != LMG_OK) return rc;
    if (kind < 0 || kind > 2 || nnz < 0 || nnz >= INT32_MAX || max_row < 0 || !d_rowptr) return LMG_ERR_ARG;
    if (nnz > 0 && (!d_colidx || !d_vals)) return LMG_ERR_ARG;
    if (max_row > kMaxCols) return LMG_ERR_CAPACITY;
    rows_fill_kernel<<<blocks(nf, kRowB), kRowB, 0, lmg_stream(stream)>>>(a, kind, d_rowptr, (int)nnz, d_colidx, d_vals);
    LMG_CHECK_LAUNCH();
    return LMG_OK;
}

}  // extern "C"
