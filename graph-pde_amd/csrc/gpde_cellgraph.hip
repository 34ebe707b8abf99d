// Radius graph by CELL LIST, emitted directly as the destination-sorted CSR the operator consumes (SURVEY.md §8 row f2
// as worded there: "cell-list / lattice-stencil; emits reference edge order or CSR directly").
//
// Replaces, together with gpde_csr_from_coo, the chain  ball_connectivity (dense float64 pairwise_distances + np.where,
// /root/reference/graph-neural-operator/utilities.py:250-255; multipole-graph-neural-operator/utilities.py:602-640)
// -> int64 COO [2, E] -> sort by destination.  gpde_radius_graph2_* (gpde_graph.hip) tests all n_src x n_dst pairs and
// writes the COO list, which gpde_csr_from_coo then radix-sorts: O(N^2) tests and 16 + 16 bytes per edge of traffic
// that the operator never needs.  Here:
//   1. the source points are binned into cubic cells of edge >= r (stable sort by cell id: ascending point id inside a cell);
//   2. one wave per DESTINATION point walks the 3^dim neighbouring cells, lanes stride over the members: pass 1 counts
//      (in-degree -> the caller's exclusive scan is `rowptr`), pass 2 writes src / dst slots straight into the CSR;
//   3. the wave sorts its row by source id in LDS (bitonic, rows up to 4096 edges), so the row is in the order a stable
//      sort by destination gives the reference's source-major edge list: rowptr / src / dst are IDENTICAL to
//      gpde_radius_graph2_* + gpde_csr_from_coo, and so are the operator's results (same summation order).
// Same two arithmetics as gpde_graph.hip (exact float64 sum of squares; GPDE_RADIUS_REFERENCE_TIES = scikit-learn's
// dot-product expansion operation by operation).  Edge attributes are addressed by CSR slot (`perm` = identity):
// generated in CSR order (synth / NodeAttr), or read from node data inside the kernel (row f3).
#include "gpde_cells.h"      // CellGrid, cell_of, sort_row_by_source: shared with gpde_knn.hip
#include <math.h>
#include <rocprim/device/device_radix_sort.hpp>

#pragma clang fp contract(off)      // the reference-ties arithmetic is defined by where it rounds

namespace {

constexpr int CG_SORT_MAX = 4096;    // rows up to this many edges are sorted by source id in LDS

__global__ void k_cell_ids(const double* __restrict__ pos, int n, CellGrid g, uint32_t* __restrict__ cell, uint32_t* __restrict__ id) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double p[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < g.dim; ++k) p[k] = pos[(size_t)j * g.dim + k];
    int c[3];
    cell_of(g, p, c);
    cell[j] = (uint32_t)((c[2] * g.nc[1] + c[1]) * g.nc[0] + c[0]);
    id[j] = (uint32_t)j;
}

// start[c] = first position in the sorted cell list whose cell id is >= c   (c = 0 .. ncells)
__global__ void k_cell_start(const uint32_t* __restrict__ sorted_cell, int n, int ncells, int32_t* __restrict__ start) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > ncells) return;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sorted_cell[mid] < (uint32_t)c) lo = mid + 1; else hi = mid;
    }
    start[c] = lo;
}

template <bool FILL, bool TIES>
__global__ __launch_bounds__(256) void k_cell_neighbors(const double* __restrict__ ps, const double* __restrict__ pd, int nd,
                                                        CellGrid g, double r2, double d2_max, int same_set,
                                                        const int32_t* __restrict__ cell_start, const uint32_t* __restrict__ order,
                                                        int32_t* __restrict__ deg, const int32_t* __restrict__ rowptr,
                                                        int32_t* __restrict__ src, int32_t* __restrict__ dst) {
    extern __shared__ uint32_t sbuf[];                  // FILL: [4 waves][CG_SORT_MAX]
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= nd) return;
    double pi[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < g.dim; ++k) pi[k] = pd[(size_t)i * g.dim + k];
    double yy = 0.0;
    if (TIES)
        for (int k = 0; k < g.dim; ++k) yy = yy + pi[k] * pi[k];
    int ci[3];
    cell_of(g, pi, ci);
    const int r0 = FILL ? rowptr[i] : 0;
    const int n_row = FILL ? rowptr[i + 1] - r0 : 0;
    const bool in_lds = FILL && n_row <= CG_SORT_MAX;
    uint32_t* row = sbuf + wave * CG_SORT_MAX;
    int count = 0;
    for (int dz = (g.dim > 2 ? -1 : 0); dz <= (g.dim > 2 ? 1 : 0); ++dz)
        for (int dy = (g.dim > 1 ? -1 : 0); dy <= (g.dim > 1 ? 1 : 0); ++dy) {
            const int cz = ci[2] + dz, cy = ci[1] + dy;
            if (cz < 0 || cz >= g.nc[2] || cy < 0 || cy >= g.nc[1]) continue;
            // the x-neighbours of a cell row are contiguous in the sorted list: one range for dx = -1 .. 1
            const int cx0 = max(ci[0] - 1, 0), cx1 = min(ci[0] + 1, g.nc[0] - 1);
            const int base = (cz * g.nc[1] + cy) * g.nc[0];
            const int p0 = cell_start[base + cx0], p1 = cell_start[base + cx1 + 1];
            for (int q0 = p0; q0 < p1; q0 += 64) {
                const int q = q0 + lane;
                bool hit = false;
                int j = 0;
                if (q < p1) {
                    j = (int)order[q];
                    if (TIES) {
                        double xx = 0.0, dot = 0.0;
                        for (int k = 0; k < g.dim; ++k) {
                            const double x = ps[(size_t)j * g.dim + k];
                            xx = xx + x * x;
                            dot = fma(x, pi[k], dot);
                        }
                        double d2 = -2.0 * dot;
                        d2 = d2 + xx;
                        d2 = d2 + yy;
                        if (d2 < 0.0) d2 = 0.0;
                        if (same_set && i == j) d2 = 0.0;
                        hit = d2 <= d2_max;
                    } else {
                        double d2 = 0.0;
                        for (int k = 0; k < g.dim; ++k) {
                            const double d = pi[k] - ps[(size_t)j * g.dim + k];
                            d2 += d * d;
                        }
                        hit = d2 <= r2;
                    }
                }
                const unsigned long long m = __ballot(hit);
                if (FILL && hit) {
                    const int slot = count + __popcll(m & ((1ull << lane) - 1ull));
                    if (slot < n_row) {
                        if (in_lds) row[slot] = (uint32_t)j;
                        else src[r0 + slot] = j;              // very long rows: cell order (deterministic, not ascending)
                    }
                }
                count += __popcll(m);
            }
        }
    if (!FILL) {
        if (lane == 0) deg[i] = count;
        return;
    }
    if (in_lds) {
        sort_row_by_source(row, n_row, lane);
        for (int t = lane; t < n_row; t += 64) src[r0 + t] = (int32_t)row[t];
    }
    for (int t = lane; t < n_row; t += 64) dst[r0 + t] = i;
}

// ---- periodic (torus) arm: gpde_radius_csr_periodic_* ---------------------------------------------------------------------
// The same cell list on a box whose axes may wrap: the reference's torus problems (TorusGridSplitter.torus_connectivity,
// torus1d_connectivity, Burgers with is_periodic) join points across the seam and feed the kernel network the WRAPPED
// displacement.  Axis k with period[k] = L > 0 is periodic from origin[k]; period[k] = 0 is an open axis (the arithmetic of
// the open kernel).  Sibling kernels: the open ones above keep their code.
//   binning   a point is reduced into [origin, origin + L) (x - L floor((x - o) / L), float64) and the reduced sources are
//             kept in the workspace; nc = floor(L / r) cells of edge L / nc >= r tile the period exactly;
//   walk      the distinct members of {c - 1, c, c + 1} mod nc, each once.  From 3 cells on, the cell across the seam is a
//             whole period away: its image shift is the same for every candidate of the cell - it moves the DESTINATION
//             (one wave-uniform value per neighbour cell) and the lanes subtract as in the open kernel.  With nc <= 2 the
//             cells c - 1 and c + 1 are one cell that holds points on both sides: visited once, nearest image per candidate;
//   distance  exact float64 sum of squares of the minimum-image differences against r^2; 2 r < L (checked on the host)
//             makes the nearest image unique, so a pair gives at most one edge;
//   geometry  optional, fill pass: geom[slot] = (pos_src[j] - image(pos_dst[i])) per axis and its norm, float64 rounded
//             once to float32 - the [dx, dy, |d|] columns of TorusGridSplitter.get_data, in slot order.
struct PeriodicGrid {
    CellGrid cells;             // lo = origin on periodic axes
    double per[3], half[3];     // period (0: open axis) and period / 2
    int wrap[3];                // 0 open, 1 periodic with >= 3 cells (one shift per neighbour cell), 2 periodic with <= 2 (per candidate)
};

__device__ __forceinline__ double reduce_into_period(double x, double o, double L) {
    return L > 0.0 ? x - L * floor((x - o) / L) : x;
}

// x_src - (the image of x_dst nearest to x_src): the image is chosen by comparison, the difference is taken once - the same
// operation the walk performs with the shift of a neighbour cell, so both give the same bits for an edge
__device__ __forceinline__ double nearest_image_diff(double xs, double xd, double L, double half) {
    const double raw = xs - xd;
    const double xim = raw > half ? xd + L : (raw < -half ? xd - L : xd);
    return xs - xim;
}

__global__ void k_cell_ids_periodic(const double* __restrict__ pos, int n, PeriodicGrid g, double* __restrict__ reduced,
                                    uint32_t* __restrict__ cell, uint32_t* __restrict__ id) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int dim = g.cells.dim;
    double p[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < dim; ++k) {
        p[k] = reduce_into_period(pos[(size_t)j * dim + k], g.cells.lo[k], g.per[k]);
        reduced[(size_t)j * dim + k] = p[k];
    }
    int c[3];
    cell_of(g.cells, p, c);
    cell[j] = (uint32_t)((c[2] * g.cells.nc[1] + c[1]) * g.cells.nc[0] + c[0]);
    id[j] = (uint32_t)j;
}

// The cells one axis contributes to the walk of a destination in cell c: a0 .. a1 as they lie, then (extra >= 0) the one
// cell across the seam, whose points are nearest after moving by `shift`.
struct AxisWalk { int a0, a1, extra; double shift; };

__device__ __forceinline__ AxisWalk axis_walk(const PeriodicGrid& g, int k, int c) {
    const int nc = g.cells.nc[k];
    AxisWalk w;
    w.extra = -1;
    w.shift = 0.0;
    if (g.wrap[k] == 2) { w.a0 = 0; w.a1 = nc - 1; return w; }         // 1 or 2 cells: all of them, once
    w.a0 = max(c - 1, 0);
    w.a1 = min(c + 1, nc - 1);
    if (g.wrap[k] == 1) {
        if (c == 0) { w.extra = nc - 1; w.shift = -g.per[k]; }         // its sources are nearest one period down
        else if (c == nc - 1) { w.extra = 0; w.shift = g.per[k]; }
    }
    return w;
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_cell_neighbors_periodic(const double* __restrict__ ps /* reduced sources */,
                                                                 const double* __restrict__ pd, int nd, PeriodicGrid g, double r2,
                                                                 const int32_t* __restrict__ cell_start, const uint32_t* __restrict__ order,
                                                                 int32_t* __restrict__ deg, const int32_t* __restrict__ rowptr,
                                                                 int32_t* __restrict__ src, int32_t* __restrict__ dst, float* __restrict__ geom) {
    extern __shared__ uint32_t sbuf[];                  // FILL: [4 waves][CG_SORT_MAX]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // provably wave-uniform: the destination, its cell and the
    const int i = blockIdx.x * 4 + wave;                                  // image shifts below live in scalar registers
    if (i >= nd) return;
    const int dim = g.cells.dim;
    double pi[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < dim) pi[k] = reduce_into_period(pd[(size_t)i * dim + k], g.cells.lo[k], g.per[k]);
    int ci[3];
    cell_of(g.cells, pi, ci);
    const int r0 = FILL ? rowptr[i] : 0;
    const int n_row = FILL ? rowptr[i + 1] - r0 : 0;
    const bool in_lds = FILL && n_row <= CG_SORT_MAX;
    const bool want_geom = FILL && geom != nullptr;
    uint32_t* row = sbuf + wave * CG_SORT_MAX;
    const AxisWalk wx = axis_walk(g, 0, ci[0]), wy = axis_walk(g, 1, ci[1]), wz = axis_walk(g, 2, ci[2]);
    double pim[3];                                      // the destination's image for the cells being walked
    int count = 0;
    for (int tz = wz.a0; tz <= wz.a1 + (wz.extra >= 0 ? 1 : 0); ++tz) {
        const int cz = tz > wz.a1 ? wz.extra : tz;
        pim[2] = tz > wz.a1 ? pi[2] - wz.shift : pi[2];
        for (int ty = wy.a0; ty <= wy.a1 + (wy.extra >= 0 ? 1 : 0); ++ty) {
            const int cy = ty > wy.a1 ? wy.extra : ty;
            pim[1] = ty > wy.a1 ? pi[1] - wy.shift : pi[1];
            const int base = (cz * g.cells.nc[1] + cy) * g.cells.nc[0];
            // the x-neighbours that lie as they are form one range of the sorted list; the cell across the seam is a second one
            for (int tx = 0; tx <= (wx.extra >= 0 ? 1 : 0); ++tx) {
                const int cx0 = tx ? wx.extra : wx.a0, cx1 = tx ? wx.extra : wx.a1;
                pim[0] = tx ? pi[0] - wx.shift : pi[0];
                const int p0 = cell_start[base + cx0], p1 = cell_start[base + cx1 + 1];
                for (int q0 = p0; q0 < p1; q0 += 64) {
                    const int q = q0 + lane;
                    bool hit = false;
                    int j = 0;
                    double d[3] = {0.0, 0.0, 0.0}, d2 = 0.0;
                    if (q < p1) {
                        j = (int)order[q];
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            if (k < dim) {
                                const double x = ps[(size_t)j * dim + k];
                                d[k] = g.wrap[k] == 2 ? nearest_image_diff(x, pi[k], g.per[k], g.half[k]) : x - pim[k];
                                d2 += d[k] * d[k];
                            }
                        hit = d2 <= r2;
                    }
                    const unsigned long long m = __ballot(hit);
                    if (FILL && hit) {
                        const int slot = count + __popcll(m & ((1ull << lane) - 1ull));
                        if (slot < n_row) {
                            if (in_lds) row[slot] = (uint32_t)j;
                            else {                            // very long rows: cell order (deterministic, not ascending)
                                src[r0 + slot] = j;
                                if (want_geom) {
                                    float* gs = geom + (size_t)(r0 + slot) * (dim + 1);
#pragma unroll
                                    for (int k = 0; k < 3; ++k)
                                        if (k < dim) gs[k] = (float)d[k];
                                    gs[dim] = (float)sqrt(d2);
                                }
                            }
                        }
                    }
                    count += __popcll(m);
                }
            }
        }
    }
    if (!FILL) {
        if (lane == 0) deg[i] = count;
        return;
    }
    if (in_lds) {
        sort_row_by_source(row, n_row, lane);
        for (int t = lane; t < n_row; t += 64) {
            const int j = (int)row[t];
            src[r0 + t] = j;
            if (want_geom) {                                  // the slot of an edge is known only now: its difference again
                float* gs = geom + (size_t)(r0 + t) * (dim + 1);
                double d2 = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < dim) {
                        const double x = ps[(size_t)j * dim + k];
                        const double dk = g.wrap[k] ? nearest_image_diff(x, pi[k], g.per[k], g.half[k]) : x - pi[k];
                        gs[k] = (float)dk;
                        d2 += dk * dk;
                    }
                gs[dim] = (float)sqrt(d2);
            }
        }
    }
    for (int t = lane; t < n_row; t += 64) dst[r0 + t] = i;
}

double sqrt_threshold(double r) {      // largest double t with sqrt(t) <= r (see gpde_graph.hip)
    double t = r * r;
    while (t > 0.0 && sqrt(t) > r) t = nextafter(t, 0.0);
    while (sqrt(nextafter(t, INFINITY)) <= r) t = nextafter(t, INFINITY);
    return t;
}

size_t al256(size_t v) { return (v + 255) / 256 * 256; }

int make_grid(int dim, double r, const double* lo, const double* hi, CellGrid* g, int64_t* ncells) {
    double cs = r * 1.0001;                      // cell edge: a pair within r is never more than one cell apart
    if (!(cs > 0.0)) cs = 1.0;
    for (;;) {
        int64_t tot = 1;
        for (int k = 0; k < 3; ++k) {
            g->lo[k] = 0.0; g->inv[k] = 0.0; g->nc[k] = 1;
            if (k < dim) {
                const double ext = hi[k] - lo[k];
                if (!(ext >= 0.0) || !isfinite(ext)) { gpde_set_error("gpde_radius_csr: bad bounds in dimension %d", k); return GPDE_EINVAL; }
                int64_t nc = (int64_t)floor(ext / cs) + 1;
                if (nc < 1) nc = 1;
                if (nc > (1 << 20)) nc = (1 << 20) + 1;      // forces a coarser grid below
                g->lo[k] = lo[k]; g->inv[k] = 1.0 / cs; g->nc[k] = (int)nc;
                tot *= nc;
            }
        }
        if (tot <= ((int64_t)1 << 24)) { *ncells = tot; break; }
        cs *= 2.0;                               // coarser cells: still correct, more candidates per destination
    }
    g->dim = dim;
    return GPDE_OK;
}

int sort_bits_for(int64_t ncells) {
    int bits = 1;
    while (((int64_t)1 << bits) < ncells) ++bits;
    return bits;
}

struct CellWs { uint32_t *cell, *id, *cell_sorted, *order; int32_t* start; void* temp; size_t temp_bytes; size_t total;
                double* reduced; /* periodic arm: the sources reduced into the period, [n_src][dim] */ };

CellWs carve(void* ws, int64_t n_src, int64_t ncells, size_t reduced_bytes = 0) {
    CellWs w{};
    size_t tb = 0;
    (void)rocprim::radix_sort_pairs(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                    (size_t)n_src, 0, sort_bits_for(ncells), (hipStream_t)0);
    char* p = (char*)(((uintptr_t)ws + 255) / 256 * 256);
    const size_t a = al256((size_t)(n_src > 0 ? n_src : 1) * 4);
    w.cell = (uint32_t*)p; p += a;
    w.id = (uint32_t*)p; p += a;
    w.cell_sorted = (uint32_t*)p; p += a;
    w.order = (uint32_t*)p; p += a;
    w.start = (int32_t*)p; p += al256((size_t)(ncells + 1) * 4);
    w.temp = p; w.temp_bytes = tb; p += al256(tb);
    w.reduced = (double*)p; p += al256(reduced_bytes);
    w.total = (size_t)(p - (char*)ws) + 256;
    return w;
}

int check(const char* what, const double* ps, int64_t ns, const double* pd, int64_t nd, int dim, double r, uint32_t flags,
          const double* lo, const double* hi) {
    if (!ps || !pd || !lo || !hi || ns < 0 || nd < 0 || ns > 0x7fffffff || nd > 0x7fffffff || dim < 1 || dim > 3 || !(r >= 0.0) ||
        (flags & ~(uint32_t)GPDE_RADIUS_REFERENCE_TIES)) {
        gpde_set_error("%s: bad argument (dim must be 1..3, flags 0 | GPDE_RADIUS_REFERENCE_TIES, host bounds lo / hi required)", what);
        return GPDE_EINVAL;
    }
    return GPDE_OK;
}

}  // namespace

// The open cell list on its own (gpde_cells.h): what gpde_radius_csr_count does before its walk, for gpde_knn.hip.
size_t gpde_cell_list_ws_bytes(int64_t n_src, int64_t ncells) { return carve(nullptr, n_src, ncells).total + 256; }

int gpde_cell_list_slots(const char* what, int64_t n_src, int64_t ncells, void* ws, size_t ws_bytes, GpdeCellSlots* out) {
    CellWs w = carve(ws, n_src, ncells);
    if (ws_bytes < w.total) { gpde_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, w.total); return GPDE_EWORKSPACE; }
    out->cell = w.cell;
    out->id = w.id;
    return GPDE_OK;
}

int gpde_cell_list_finish(const char* what, int64_t n_src, int64_t ncells, void* ws, size_t ws_bytes, hipStream_t st, GpdeCellList* out) {
    CellWs w = carve(ws, n_src, ncells);
    if (ws_bytes < w.total) { gpde_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, w.total); return GPDE_EWORKSPACE; }
    const int T = 256;
    if (n_src > 0)
        GP_HIP_CHECK(rocprim::radix_sort_pairs(w.temp, w.temp_bytes, w.cell, w.cell_sorted, w.id, w.order, (size_t)n_src, 0,
                                               sort_bits_for(ncells), st));
    hipLaunchKernelGGL(k_cell_start, dim3((unsigned)((ncells + 1 + T - 1) / T)), dim3(T), 0, st, w.cell_sorted, (int)n_src, (int)ncells, w.start);
    out->start = w.start;
    out->order = w.order;
    return GPDE_OK;
}

int gpde_cell_list_build(const char* what, const double* pos_src, int64_t n_src, const CellGrid& g, int64_t ncells, void* ws,
                         size_t ws_bytes, hipStream_t st, GpdeCellList* out) {
    GpdeCellSlots s;
    if (int rc = gpde_cell_list_slots(what, n_src, ncells, ws, ws_bytes, &s)) return rc;
    if (n_src > 0)
        hipLaunchKernelGGL(k_cell_ids, dim3((unsigned)((n_src + 255) / 256)), dim3(256), 0, st, pos_src, (int)n_src, g, s.cell, s.id);
    return gpde_cell_list_finish(what, n_src, ncells, ws, ws_bytes, st, out);
}

extern "C" size_t gpde_radius_csr_workspace_bytes(int64_t n_src, int dim, double r, const double* lo, const double* hi) {
    CellGrid g;
    int64_t ncells = 0;
    if (n_src < 0 || dim < 1 || dim > 3 || !lo || !hi || make_grid(dim, r, lo, hi, &g, &ncells) != GPDE_OK) return 0;
    return carve(nullptr, n_src, ncells).total + 256;
}

extern "C" int gpde_radius_csr_count(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                                     double r, uint32_t flags, const double* lo, const double* hi, int32_t* deg, void* ws,
                                     size_t ws_bytes, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    if (int rc = check("gpde_radius_csr_count", pos_src, n_src, pos_dst, n_dst, dim, r, flags, lo, hi)) return rc;
    if (!deg || !ws) { gpde_set_error("gpde_radius_csr_count: deg / ws is null"); return GPDE_EINVAL; }
    CellGrid g;
    int64_t ncells = 0;
    if (int rc = make_grid(dim, r, lo, hi, &g, &ncells)) return rc;
    CellWs w = carve(ws, n_src, ncells);
    if (ws_bytes < w.total) { gpde_set_error("gpde_radius_csr_count: workspace %zu < %zu bytes", ws_bytes, w.total); return GPDE_EWORKSPACE; }
    if (n_dst == 0) return GPDE_OK;
    GpdeCellList cl;
    if (int rc = gpde_cell_list_build("gpde_radius_csr_count", pos_src, n_src, g, ncells, ws, ws_bytes, st, &cl)) return rc;
    const int same = pos_src == pos_dst && n_src == n_dst;
    const dim3 grid((unsigned)((n_dst + 3) / 4)), block(256);
    if (flags & GPDE_RADIUS_REFERENCE_TIES)
        hipLaunchKernelGGL((k_cell_neighbors<false, true>), grid, block, 0, st, pos_src, pos_dst, (int)n_dst, g, r * r, sqrt_threshold(r),
                           same, w.start, w.order, deg, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
    else
        hipLaunchKernelGGL((k_cell_neighbors<false, false>), grid, block, 0, st, pos_src, pos_dst, (int)n_dst, g, r * r, sqrt_threshold(r),
                           same, w.start, w.order, deg, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
    GP_LAUNCH_CHECK("gpde_radius_csr_count kernels");
    return GPDE_OK;
}

// `ws` must still hold what gpde_radius_csr_count left there (same arguments); rowptr = exclusive scan of its `deg`.
extern "C" int gpde_radius_csr_fill(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                                    double r, uint32_t flags, const double* lo, const double* hi, const int32_t* rowptr,
                                    int32_t* src, int32_t* dst, int64_t n_edges, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    if (int rc = check("gpde_radius_csr_fill", pos_src, n_src, pos_dst, n_dst, dim, r, flags, lo, hi)) return rc;
    if (!rowptr || !ws || (n_edges > 0 && (!src || !dst))) { gpde_set_error("gpde_radius_csr_fill: null rowptr / src / dst / ws"); return GPDE_EINVAL; }
    CellGrid g;
    int64_t ncells = 0;
    if (int rc = make_grid(dim, r, lo, hi, &g, &ncells)) return rc;
    CellWs w = carve(ws, n_src, ncells);
    if (ws_bytes < w.total) { gpde_set_error("gpde_radius_csr_fill: workspace %zu < %zu bytes", ws_bytes, w.total); return GPDE_EWORKSPACE; }
    if (n_dst == 0 || n_edges == 0) return GPDE_OK;
    const int same = pos_src == pos_dst && n_src == n_dst;
    const dim3 grid((unsigned)((n_dst + 3) / 4)), block(256);
    const size_t lds = (size_t)4 * CG_SORT_MAX * 4;
    if (flags & GPDE_RADIUS_REFERENCE_TIES)
        hipLaunchKernelGGL((k_cell_neighbors<true, true>), grid, block, lds, st, pos_src, pos_dst, (int)n_dst, g, r * r, sqrt_threshold(r),
                           same, w.start, w.order, (int32_t*)nullptr, rowptr, src, dst);
    else
        hipLaunchKernelGGL((k_cell_neighbors<true, false>), grid, block, lds, st, pos_src, pos_dst, (int)n_dst, g, r * r, sqrt_threshold(r),
                           same, w.start, w.order, (int32_t*)nullptr, rowptr, src, dst);
    GP_LAUNCH_CHECK("gpde_radius_csr_fill kernels");
    return GPDE_OK;
}

// ---- periodic arm: host side ------------------------------------------------------------------------------------------------
namespace {

// Every argument error of the periodic entry points that the scalars and the two host arrays show, before anything else is looked at.
int check_periodic(const char* what, int dim, double r, const double* origin, const double* period) {
    if (dim < 1 || dim > 3) { gpde_set_error("%s: dim must be 1..3 (got %d)", what, dim); return GPDE_EINVAL; }
    if (!origin || !period) { gpde_set_error("%s: host arrays origin[dim] / period[dim] required", what); return GPDE_EINVAL; }
    if (!(r > 0.0) || !isfinite(r)) { gpde_set_error("%s: r must be positive and finite", what); return GPDE_EINVAL; }
    for (int k = 0; k < dim; ++k) {
        if (!(period[k] >= 0.0) || !isfinite(period[k]) || !isfinite(origin[k])) {
            gpde_set_error("%s: period[%d] must be >= 0 (0 = open axis) and origin[%d] finite", what, k, k);
            return GPDE_EINVAL;
        }
        if (period[k] > 0.0 && !(2.0 * r < period[k])) {
            gpde_set_error("%s: 2 r = %g >= period[%d] = %g: a pair would have more than one image within r", what, 2.0 * r, k, period[k]);
            return GPDE_EINVAL;
        }
    }
    return GPDE_OK;
}

// Cells of a periodic axis tile the period exactly: nc = floor(L / r) of edge L / nc >= r.  Where that edge is within 2^-20 of r
// (L / r an integer, or next to one) one cell fewer is taken: the cell index is a rounded product, and with an edge of exactly r
// a pair at distance r(1 - 1e-16) could land two cells apart.  Open axes are those of make_grid.  Too many cells: coarser ones.
int make_periodic_grid(const char* what, int dim, double r, const double* lo, const double* hi, const double* origin,
                       const double* period, PeriodicGrid* g, int64_t* ncells) {
    for (double scale = 1.0;; scale *= 2.0) {
        int64_t tot = 1;
        for (int k = 0; k < 3; ++k) {
            g->cells.lo[k] = 0.0; g->cells.inv[k] = 0.0; g->cells.nc[k] = 1;
            g->per[k] = 0.0; g->half[k] = 0.0; g->wrap[k] = 0;
            if (k >= dim) continue;
            int64_t nc;
            if (period[k] > 0.0) {
                const double L = period[k], edge_min = r * scale * (1.0 + 0x1p-20);
                nc = (int64_t)fmin(floor(L / (r * scale)), (double)((1 << 20) + 1));
                while (nc > 1 && L / (double)nc < edge_min) --nc;
                if (nc < 1) nc = 1;
                g->cells.lo[k] = origin[k]; g->cells.inv[k] = (double)nc / L;
                g->per[k] = L; g->half[k] = 0.5 * L; g->wrap[k] = nc >= 3 ? 1 : 2;
            } else {
                if (!lo || !hi) { gpde_set_error("%s: an open axis needs the host bounds lo / hi", what); return GPDE_EINVAL; }
                const double ext = hi[k] - lo[k], cs = r * 1.0001 * scale;
                if (!(ext >= 0.0) || !isfinite(ext)) { gpde_set_error("%s: bad bounds in dimension %d", what, k); return GPDE_EINVAL; }
                nc = (int64_t)fmin(floor(ext / cs), (double)(1 << 20)) + 1;
                g->cells.lo[k] = lo[k]; g->cells.inv[k] = 1.0 / cs;
            }
            g->cells.nc[k] = (int)nc;
            tot *= nc;
        }
        if (tot <= ((int64_t)1 << 24)) { *ncells = tot; break; }
    }
    g->cells.dim = dim;
    return GPDE_OK;
}

int check_periodic_points(const char* what, const double* ps, int64_t ns, const double* pd, int64_t nd, uint32_t flags) {
    if (flags & GPDE_RADIUS_REFERENCE_TIES) {
        gpde_set_error("%s: GPDE_RADIUS_REFERENCE_TIES has no periodic form (the reference's torus code never wraps: nothing to reproduce)", what);
        return GPDE_EINVAL;
    }
    if (flags || !ps || !pd || ns < 0 || nd < 0 || ns > 0x7fffffff || nd > 0x7fffffff) {
        gpde_set_error("%s: bad argument (flags must be 0, positions non-null, 0 <= n <= 2^31 - 1)", what);
        return GPDE_EINVAL;
    }
    return GPDE_OK;
}

}  // namespace

extern "C" size_t gpde_radius_csr_periodic_workspace_bytes(int64_t n_src, int dim, double r, const double* lo, const double* hi,
                                                           const double* origin, const double* period) {
    const char* what = "gpde_radius_csr_periodic_workspace_bytes";
    PeriodicGrid g;
    int64_t ncells = 0;
    if (check_periodic(what, dim, r, origin, period) != GPDE_OK) return 0;
    if (n_src < 0 || n_src > 0x7fffffff) { gpde_set_error("%s: n_src out of range", what); return 0; }
    if (make_periodic_grid(what, dim, r, lo, hi, origin, period, &g, &ncells) != GPDE_OK) return 0;
    return carve(nullptr, n_src, ncells, (size_t)(n_src > 0 ? n_src : 1) * dim * sizeof(double)).total + 256;
}

extern "C" int gpde_radius_csr_periodic_count(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                                              double r, uint32_t flags, const double* lo, const double* hi, const double* origin,
                                              const double* period, int32_t* deg, void* ws, size_t ws_bytes, void* stream_) {
    const char* what = "gpde_radius_csr_periodic_count";
    hipStream_t st = (hipStream_t)stream_;
    if (int rc = check_periodic(what, dim, r, origin, period)) return rc;
    if (int rc = check_periodic_points(what, pos_src, n_src, pos_dst, n_dst, flags)) return rc;
    if (!deg || !ws) { gpde_set_error("%s: deg / ws is null", what); return GPDE_EINVAL; }
    PeriodicGrid g;
    int64_t ncells = 0;
    if (int rc = make_periodic_grid(what, dim, r, lo, hi, origin, period, &g, &ncells)) return rc;
    CellWs w = carve(ws, n_src, ncells, (size_t)(n_src > 0 ? n_src : 1) * dim * sizeof(double));
    if (ws_bytes < w.total) { gpde_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, w.total); return GPDE_EWORKSPACE; }
    if (n_dst == 0) return GPDE_OK;
    const int T = 256;
    if (n_src > 0) {
        hipLaunchKernelGGL(k_cell_ids_periodic, dim3((unsigned)((n_src + T - 1) / T)), dim3(T), 0, st, pos_src, (int)n_src, g, w.reduced,
                           w.cell, w.id);
        GP_HIP_CHECK(rocprim::radix_sort_pairs(w.temp, w.temp_bytes, w.cell, w.cell_sorted, w.id, w.order, (size_t)n_src, 0,
                                               sort_bits_for(ncells), st));
    }
    hipLaunchKernelGGL(k_cell_start, dim3((unsigned)((ncells + 1 + T - 1) / T)), dim3(T), 0, st, w.cell_sorted, (int)n_src, (int)ncells, w.start);
    hipLaunchKernelGGL((k_cell_neighbors_periodic<false>), dim3((unsigned)((n_dst + 3) / 4)), dim3(256), 0, st, w.reduced, pos_dst, (int)n_dst,
                       g, r * r, w.start, w.order, deg, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr);
    GP_LAUNCH_CHECK("gpde_radius_csr_periodic_count kernels");
    return GPDE_OK;
}

// `ws` must still hold what gpde_radius_csr_periodic_count left there (same arguments); rowptr = exclusive scan of its `deg`.
extern "C" int gpde_radius_csr_periodic_fill(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                                             double r, uint32_t flags, const double* lo, const double* hi, const double* origin,
                                             const double* period, const int32_t* rowptr, int32_t* src, int32_t* dst, float* geom,
                                             int64_t n_edges, void* ws, size_t ws_bytes, void* stream_) {
    const char* what = "gpde_radius_csr_periodic_fill";
    hipStream_t st = (hipStream_t)stream_;
    if (int rc = check_periodic(what, dim, r, origin, period)) return rc;
    if (int rc = check_periodic_points(what, pos_src, n_src, pos_dst, n_dst, flags)) return rc;
    if (!rowptr || !ws || n_edges < 0 || (n_edges > 0 && (!src || !dst))) { gpde_set_error("%s: null rowptr / src / dst / ws", what); return GPDE_EINVAL; }
    PeriodicGrid g;
    int64_t ncells = 0;
    if (int rc = make_periodic_grid(what, dim, r, lo, hi, origin, period, &g, &ncells)) return rc;
    CellWs w = carve(ws, n_src, ncells, (size_t)(n_src > 0 ? n_src : 1) * dim * sizeof(double));
    if (ws_bytes < w.total) { gpde_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, w.total); return GPDE_EWORKSPACE; }
    if (n_dst == 0 || n_edges == 0) return GPDE_OK;
    hipLaunchKernelGGL((k_cell_neighbors_periodic<true>), dim3((unsigned)((n_dst + 3) / 4)), dim3(256), (size_t)4 * CG_SORT_MAX * 4, st, w.reduced,
                       pos_dst, (int)n_dst, g, r * r, w.start, w.order, (int32_t*)nullptr, rowptr, src, dst, geom);
    GP_LAUNCH_CHECK("gpde_radius_csr_periodic_fill kernels");
    return GPDE_OK;
}

// ---- batched arm: gpde_radius_csr_batched_* -----------------------------------------------------------------------------------
// The radius graphs of B independent point sets in ONE build: the block-diagonal destination CSR with global node ids.  The
// reference's training scripts build one small graph per sample in a Python loop (UAI3_resolution.py:131-145,
// neurips1_MGKN.py:204) and the DataLoader collates them; one call of the open builder per sample costs two host
// synchronisations, a radix sort and four launches each.  Sibling kernels: the open and periodic ones above keep their code.
//   table     one BatchGraph record per graph (GPDE_RADIUS_BATCHED_REC_BYTES), written on the HOST by
//             gpde_radius_csr_batched_plan and handed to count / fill in a device buffer: the graph's own CellGrid (the rule of
//             make_grid on its own bounds and radius), r^2 and the reference-ties threshold, its first cell `cell_base` in the
//             batch-wide cell numbering, and its source / destination ranges of the concatenated position arrays;
//   keys      source j of graph b sorts under cell_base[b] + (its cell in b's grid): one stable radix sort orders all sources
//             graph-major, cell-major, ascending id inside a cell; one k_cell_start runs over the summed cell count;
//   walk      one wave per destination: binary search of its graph in the table (wave-uniform), then the 3^dim cells of that
//             graph only - the contiguous x-range is taken from the graph's own base, so it never runs into the next graph's
//             cells.  Arithmetic, ballot slots, LDS row sort and the cell-order fallback are those of k_cell_neighbors;
//   cap       the summed cell count is held to BATCH_CELL_CAP = 2^24 (make_grid's own cap for one graph, so B = 1 plans the
//             grid of the open builder): while it is exceeded every graph's cell edge doubles (a coarser filter, same edges).
//             A batch of more graphs than that ends at one cell per graph.
namespace {

struct BatchGraph {
    double lo[3], inv[3];
    double r2, d2_max;
    int32_t nc[3];
    int32_t cell_base;
    int32_t src_begin, src_end, dst_begin, dst_end;
};
static_assert(sizeof(BatchGraph) == GPDE_RADIUS_BATCHED_REC_BYTES, "BatchGraph is the record of include/gpde.h");

constexpr int64_t BATCH_CELL_CAP = (int64_t)1 << 24;

// the graph that owns point `p`: the first record whose range ends after p (empty graphs in between are passed over)
template <bool DST>
__device__ __forceinline__ int graph_of(const BatchGraph* __restrict__ tab, int n_graphs, int p) {
    int lo = 0, hi = n_graphs - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((DST ? tab[mid].dst_end : tab[mid].src_end) <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ CellGrid grid_of(const BatchGraph& t, int dim) {
    CellGrid g;
#pragma unroll
    for (int k = 0; k < 3; ++k) { g.lo[k] = t.lo[k]; g.inv[k] = t.inv[k]; g.nc[k] = t.nc[k]; }
    g.dim = dim;
    return g;
}

__global__ void k_cell_ids_batched(const double* __restrict__ pos, int n, int dim, const BatchGraph* __restrict__ tab, int n_graphs,
                                   uint32_t* __restrict__ cell, uint32_t* __restrict__ id) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const BatchGraph t = tab[graph_of<false>(tab, n_graphs, j)];
    const CellGrid g = grid_of(t, dim);
    double p[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < dim; ++k) p[k] = pos[(size_t)j * dim + k];
    int c[3];
    cell_of(g, p, c);
    cell[j] = (uint32_t)(t.cell_base + (c[2] * g.nc[1] + c[1]) * g.nc[0] + c[0]);
    id[j] = (uint32_t)j;
}

template <bool FILL, bool TIES>
__global__ __launch_bounds__(256) void k_cell_neighbors_batched(const double* __restrict__ ps, const double* __restrict__ pd, int nd, int dim,
                                                                const BatchGraph* __restrict__ tab, int n_graphs, int n_cells, int same_set,
                                                                const int32_t* __restrict__ cell_start, const uint32_t* __restrict__ order,
                                                                int32_t* __restrict__ deg, const int32_t* __restrict__ rowptr,
                                                                int32_t* __restrict__ src, int32_t* __restrict__ dst) {
    extern __shared__ uint32_t sbuf[];                  // FILL: [4 waves][CG_SORT_MAX]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: the graph search and its record are scalar
    const int i = blockIdx.x * 4 + wave;
    if (i >= nd) return;
    const BatchGraph t = tab[graph_of<true>(tab, n_graphs, i)];
    const CellGrid g = grid_of(t, dim);
    const double r2 = t.r2, d2_max = t.d2_max;
    double pi[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < g.dim; ++k) pi[k] = pd[(size_t)i * g.dim + k];
    double yy = 0.0;
    if (TIES)
        for (int k = 0; k < g.dim; ++k) yy = yy + pi[k] * pi[k];
    int ci[3];
    cell_of(g, pi, ci);
    const int r0 = FILL ? rowptr[i] : 0;
    const int n_row = FILL ? rowptr[i + 1] - r0 : 0;
    const bool in_lds = FILL && n_row <= CG_SORT_MAX;
    uint32_t* row = sbuf + wave * CG_SORT_MAX;
    int count = 0;
    for (int dz = (g.dim > 2 ? -1 : 0); dz <= (g.dim > 2 ? 1 : 0); ++dz)
        for (int dy = (g.dim > 1 ? -1 : 0); dy <= (g.dim > 1 ? 1 : 0); ++dy) {
            const int cz = ci[2] + dz, cy = ci[1] + dy;
            if (cz < 0 || cz >= g.nc[2] || cy < 0 || cy >= g.nc[1]) continue;
            // the x-neighbours of a cell row are contiguous in the sorted list: one range for dx = -1 .. 1, inside THIS graph's cells
            const int cx0 = max(ci[0] - 1, 0), cx1 = min(ci[0] + 1, g.nc[0] - 1);
            const int base = t.cell_base + (cz * g.nc[1] + cy) * g.nc[0];
            if (base < 0 || base + cx1 + 1 > n_cells) continue;       // a table that does not belong to this workspace reads nothing
            const int p0 = cell_start[base + cx0], p1 = cell_start[base + cx1 + 1];
            for (int q0 = p0; q0 < p1; q0 += 64) {
                const int q = q0 + lane;
                bool hit = false;
                int j = 0;
                if (q < p1) {
                    j = (int)order[q];
                    if (TIES) {
                        double xx = 0.0, dot = 0.0;
                        for (int k = 0; k < g.dim; ++k) {
                            const double x = ps[(size_t)j * g.dim + k];
                            xx = xx + x * x;
                            dot = fma(x, pi[k], dot);
                        }
                        double d2 = -2.0 * dot;
                        d2 = d2 + xx;
                        d2 = d2 + yy;
                        if (d2 < 0.0) d2 = 0.0;
                        if (same_set && i == j) d2 = 0.0;             // global ids: one point set, the diagonal of its own graph
                        hit = d2 <= d2_max;
                    } else {
                        double d2 = 0.0;
                        for (int k = 0; k < g.dim; ++k) {
                            const double d = pi[k] - ps[(size_t)j * g.dim + k];
                            d2 += d * d;
                        }
                        hit = d2 <= r2;
                    }
                }
                const unsigned long long m = __ballot(hit);
                if (FILL && hit) {
                    const int slot = count + __popcll(m & ((1ull << lane) - 1ull));
                    if (slot < n_row) {
                        if (in_lds) row[slot] = (uint32_t)j;
                        else src[r0 + slot] = j;              // very long rows: cell order (deterministic, not ascending)
                    }
                }
                count += __popcll(m);
            }
        }
    if (!FILL) {
        if (lane == 0) deg[i] = count;
        return;
    }
    if (in_lds) {
        sort_row_by_source(row, n_row, lane);
        for (int t2 = lane; t2 < n_row; t2 += 64) src[r0 + t2] = (int32_t)row[t2];
    }
    for (int t2 = lane; t2 < n_row; t2 += 64) dst[r0 + t2] = i;
}

// ptr[0] = 0 <= ptr[1] <= ... <= ptr[B] = n <= 2^31 - 1
int check_ptr(const char* what, const char* name, const int64_t* ptr, int64_t n_graphs, int64_t n) {
    if (!ptr) { gpde_set_error("%s: host array %s[n_graphs + 1] required", what, name); return GPDE_EINVAL; }
    if (ptr[0] != 0) { gpde_set_error("%s: %s[0] = %lld, must be 0", what, name, (long long)ptr[0]); return GPDE_EINVAL; }
    for (int64_t b = 0; b < n_graphs; ++b)
        if (ptr[b + 1] < ptr[b]) {
            gpde_set_error("%s: %s decreases at graph %lld (%lld -> %lld)", what, name, (long long)b, (long long)ptr[b], (long long)ptr[b + 1]);
            return GPDE_EINVAL;
        }
    if (ptr[n_graphs] > 0x7fffffff) { gpde_set_error("%s: %s ends at %lld points, more than 2^31 - 1", what, name, (long long)ptr[n_graphs]); return GPDE_EINVAL; }
    if (n >= 0 && ptr[n_graphs] != n) {
        gpde_set_error("%s: %s ends at %lld, the position array has %lld points", what, name, (long long)ptr[n_graphs], (long long)n);
        return GPDE_EINVAL;
    }
    return GPDE_OK;
}

int check_batch_scalars(const char* what, int64_t n_graphs, int dim) {
    if (dim < 1 || dim > 3) { gpde_set_error("%s: dim must be 1..3 (got %d)", what, dim); return GPDE_EINVAL; }
    if (n_graphs < 0 || n_graphs > 0x7ffffffe) { gpde_set_error("%s: n_graphs = %lld out of range (0 .. 2^31 - 2)", what, (long long)n_graphs); return GPDE_EINVAL; }
    return GPDE_OK;
}

// what count and fill share: every refusal the host values show, then the workspace carved for n_cells
int check_batched_call(const char* what, const double* ps, int64_t ns, const double* pd, int64_t nd, int dim, uint32_t flags,
                       const int64_t* ptr_src, const int64_t* ptr_dst, int64_t n_graphs, const void* table, int64_t n_cells,
                       void* ws, size_t ws_bytes, CellWs* w) {
    if (int rc = check_batch_scalars(what, n_graphs, dim)) return rc;
    if (flags & ~(uint32_t)GPDE_RADIUS_REFERENCE_TIES) { gpde_set_error("%s: flags must be 0 | GPDE_RADIUS_REFERENCE_TIES", what); return GPDE_EINVAL; }
    if (ns < 0 || nd < 0 || ns > 0x7fffffff || nd > 0x7fffffff) { gpde_set_error("%s: point counts must be 0 .. 2^31 - 1", what); return GPDE_EINVAL; }
    if ((ns > 0 && !ps) || (nd > 0 && !pd)) { gpde_set_error("%s: pos_src / pos_dst is null", what); return GPDE_EINVAL; }
    if (int rc = check_ptr(what, "ptr_src", ptr_src, n_graphs, ns)) return rc;
    if (int rc = check_ptr(what, "ptr_dst", ptr_dst, n_graphs, nd)) return rc;
    if (ps == pd && ns == nd)                              // ONE point set: one division into graphs
        for (int64_t b = 0; b <= n_graphs; ++b)
            if (ptr_dst[b] != ptr_src[b]) {
                gpde_set_error("%s: pos_dst is pos_src (one point set) but ptr_dst[%lld] = %lld differs from ptr_src[%lld] = %lld", what,
                               (long long)b, (long long)ptr_dst[b], (long long)b, (long long)ptr_src[b]);
                return GPDE_EINVAL;
            }
    if (n_graphs > 0 && !table) { gpde_set_error("%s: the device table of gpde_radius_csr_batched_plan is null", what); return GPDE_EINVAL; }
    if (n_cells < n_graphs || n_cells > 0x7ffffffe) { gpde_set_error("%s: n_cells = %lld is not what the plan returned for %lld graphs", what, (long long)n_cells, (long long)n_graphs); return GPDE_EINVAL; }
    if (!ws) { gpde_set_error("%s: ws is null", what); return GPDE_EINVAL; }
    *w = carve(ws, ns, n_cells);
    if (ws_bytes < w->total) { gpde_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, w->total); return GPDE_EWORKSPACE; }
    return GPDE_OK;
}

}  // namespace

int gpde_batch_check_ptr(const char* what, const char* name, const int64_t* ptr, int64_t n_graphs, int64_t n) {
    return check_ptr(what, name, ptr, n_graphs, n);
}

// HOST ONLY.  bounds [B][2][dim] (lo then hi of graph b; not read for a graph without sources), ptr_src / ptr_dst [B + 1]
// (ptr_dst NULL: one point set), r [B].  table (nullable: a query) receives B records.
extern "C" int gpde_radius_csr_batched_plan(const double* bounds, const int64_t* ptr_src, const int64_t* ptr_dst, const double* r,
                                            int64_t n_graphs, int dim, void* table, int64_t* n_cells, size_t* ws_bytes) {
    const char* what = "gpde_radius_csr_batched_plan";
    if (int rc = check_batch_scalars(what, n_graphs, dim)) return rc;
    if (!n_cells || !ws_bytes) { gpde_set_error("%s: n_cells / ws_bytes is null", what); return GPDE_EINVAL; }
    if (int rc = check_ptr(what, "ptr_src", ptr_src, n_graphs, -1)) return rc;
    if (!ptr_dst) ptr_dst = ptr_src;
    if (int rc = check_ptr(what, "ptr_dst", ptr_dst, n_graphs, -1)) return rc;
    if (n_graphs > 0 && (!bounds || !r)) { gpde_set_error("%s: host arrays bounds[n_graphs][2][dim] / r[n_graphs] required", what); return GPDE_EINVAL; }
    for (int64_t b = 0; b < n_graphs; ++b)
        if (!(r[b] > 0.0) || !isfinite(r[b])) { gpde_set_error("%s: r[%lld] = %g must be positive and finite", what, (long long)b, r[b]); return GPDE_EINVAL; }
    BatchGraph* tab = (BatchGraph*)table;
    int64_t total = 0;
    for (double scale = 1.0;; scale *= 2.0) {              // a power of two: r * scale * 1.0001 is make_grid's r * 1.0001 doubled
        total = 0;
        for (int64_t b = 0; b < n_graphs; ++b) {
            CellGrid g;
            int64_t nc = 1;
            if (ptr_src[b + 1] > ptr_src[b]) {
                if (int rc = make_grid(dim, r[b] * scale, bounds + (size_t)b * 2 * dim, bounds + ((size_t)b * 2 + 1) * dim, &g, &nc)) return rc;
            } else {                                       // no sources: one empty cell, whatever the bounds hold
                for (int k = 0; k < 3; ++k) { g.lo[k] = 0.0; g.inv[k] = 0.0; g.nc[k] = 1; }
            }
            if (tab) {
                BatchGraph& t = tab[b];
                for (int k = 0; k < 3; ++k) { t.lo[k] = g.lo[k]; t.inv[k] = g.inv[k]; t.nc[k] = g.nc[k]; }
                t.r2 = r[b] * r[b];
                t.d2_max = sqrt_threshold(r[b]);
                t.cell_base = (int32_t)total;
                t.src_begin = (int32_t)ptr_src[b]; t.src_end = (int32_t)ptr_src[b + 1];
                t.dst_begin = (int32_t)ptr_dst[b]; t.dst_end = (int32_t)ptr_dst[b + 1];
            }
            total += nc;
            if (total > BATCH_CELL_CAP && total > n_graphs) break;      // over the cap already: coarsen (every graph) and start over
        }
        if (total <= BATCH_CELL_CAP || total <= n_graphs) break;        // one cell per graph cannot be coarsened further
    }
    *n_cells = total;
    *ws_bytes = carve(nullptr, ptr_src[n_graphs], total).total + 256;
    return GPDE_OK;
}

extern "C" int gpde_radius_csr_batched_count(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                                             uint32_t flags, const int64_t* ptr_src, const int64_t* ptr_dst, int64_t n_graphs,
                                             const void* table, int64_t n_cells, int32_t* deg, void* ws, size_t ws_bytes, void* stream_) {
    const char* what = "gpde_radius_csr_batched_count";
    hipStream_t st = (hipStream_t)stream_;
    CellWs w;
    if (int rc = check_batched_call(what, pos_src, n_src, pos_dst, n_dst, dim, flags, ptr_src, ptr_dst, n_graphs, table, n_cells, ws, ws_bytes, &w)) return rc;
    if (n_dst > 0 && !deg) { gpde_set_error("%s: deg is null", what); return GPDE_EINVAL; }
    if (n_dst == 0) return GPDE_OK;
    const BatchGraph* tab = (const BatchGraph*)table;
    const int T = 256;
    if (n_src > 0) {
        hipLaunchKernelGGL(k_cell_ids_batched, dim3((unsigned)((n_src + T - 1) / T)), dim3(T), 0, st, pos_src, (int)n_src, dim, tab, (int)n_graphs,
                           w.cell, w.id);
        GP_HIP_CHECK(rocprim::radix_sort_pairs(w.temp, w.temp_bytes, w.cell, w.cell_sorted, w.id, w.order, (size_t)n_src, 0,
                                               sort_bits_for(n_cells), st));
    }
    hipLaunchKernelGGL(k_cell_start, dim3((unsigned)((n_cells + 1 + T - 1) / T)), dim3(T), 0, st, w.cell_sorted, (int)n_src, (int)n_cells, w.start);
    const int same = pos_src == pos_dst && n_src == n_dst;
    const dim3 grid((unsigned)((n_dst + 3) / 4)), block(256);
    if (flags & GPDE_RADIUS_REFERENCE_TIES)
        hipLaunchKernelGGL((k_cell_neighbors_batched<false, true>), grid, block, 0, st, pos_src, pos_dst, (int)n_dst, dim, tab, (int)n_graphs,
                           (int)n_cells, same, w.start, w.order, deg, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
    else
        hipLaunchKernelGGL((k_cell_neighbors_batched<false, false>), grid, block, 0, st, pos_src, pos_dst, (int)n_dst, dim, tab, (int)n_graphs,
                           (int)n_cells, same, w.start, w.order, deg, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
    GP_LAUNCH_CHECK("gpde_radius_csr_batched_count kernels");
    return GPDE_OK;
}

// `ws` must still hold what gpde_radius_csr_batched_count left there (same arguments); rowptr = exclusive scan of its `deg`.
extern "C" int gpde_radius_csr_batched_fill(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                                            uint32_t flags, const int64_t* ptr_src, const int64_t* ptr_dst, int64_t n_graphs,
                                            const void* table, int64_t n_cells, const int32_t* rowptr, int32_t* src, int32_t* dst,
                                            int64_t n_edges, void* ws, size_t ws_bytes, void* stream_) {
    const char* what = "gpde_radius_csr_batched_fill";
    hipStream_t st = (hipStream_t)stream_;
    CellWs w;
    if (int rc = check_batched_call(what, pos_src, n_src, pos_dst, n_dst, dim, flags, ptr_src, ptr_dst, n_graphs, table, n_cells, ws, ws_bytes, &w)) return rc;
    if (!rowptr || n_edges < 0 || (n_edges > 0 && (!src || !dst))) { gpde_set_error("%s: null rowptr / src / dst", what); return GPDE_EINVAL; }
    if (n_dst == 0 || n_edges == 0) return GPDE_OK;
    const BatchGraph* tab = (const BatchGraph*)table;
    const int same = pos_src == pos_dst && n_src == n_dst;
    const dim3 grid((unsigned)((n_dst + 3) / 4)), block(256);
    const size_t lds = (size_t)4 * CG_SORT_MAX * 4;
    if (flags & GPDE_RADIUS_REFERENCE_TIES)
        hipLaunchKernelGGL((k_cell_neighbors_batched<true, true>), grid, block, lds, st, pos_src, pos_dst, (int)n_dst, dim, tab, (int)n_graphs,
                           (int)n_cells, same, w.start, w.order, (int32_t*)nullptr, rowptr, src, dst);
    else
        hipLaunchKernelGGL((k_cell_neighbors_batched<true, false>), grid, block, lds, st, pos_src, pos_dst, (int)n_dst, dim, tab, (int)n_graphs,
                           (int)n_cells, same, w.start, w.order, (int32_t*)nullptr, rowptr, src, dst);
    GP_LAUNCH_CHECK("gpde_radius_csr_batched_fill kernels");
    return GPDE_OK;
}

// ---- sampled arm: gpde_gaussian_csr_* -------------------------------------------------------------------------------------------
// The reference's SECOND connectivity (gaussian_connectivity, graph-neural-operator/utilities.py:257-263, 372-378;
// multipole-graph-neural-operator/utilities.py:283-289, 419-425): every ordered pair is kept independently with probability
// exp(-d^2 / sigma^2).  Here the draw is a pure function of (seed, destination id, source id) - the counter-based hash of
// gpde_edge_keys_hash - so COUNT and FILL evaluate the same predicate and the graph depends on positions, sigma and seed only:
//     edge j -> i  iff  u(seed, i, j) < exp(-(d2 / (sigma * sigma)))          (float64, round to nearest, contraction off)
//     u   = ((double)(key >> 10) + 0.5) * 2^-53,   key = the value gpde_edge_keys_hash gives for (seed, dst = i, src = j)
//     d2  = the value gpde_edge_keys_sqdist gives for the edge, bit for bit: open axes d = x_dst - x_src, periodic axes
//           d = x_src - x_dst, d -= L rint(d / L) on the RAW coordinates; squares summed in axis order.
// u >= 2^-54, so a pair with exp(-d2 / sigma^2) <= 2^-54 is never kept: the graph lies inside the radius graph of
// r_support = sigma sqrt(54 ln 2), and a cell list of that edge (or of the optional cutoff, if smaller) is exact.  The walk is
// the periodic builder's (an open box is the case "no axis wraps"); the cells only ENUMERATE candidates - on a periodic axis they
// bin the reduced coordinates while the distance is taken from the raw ones, a few ulp apart, far inside the 2^-20 slack of the
// cell edge.  The candidate graph is never formed: at sigma = 0.1 on the 241^2 lattice it would hold 2.13e9 edges, the kept one 9.4e7.
//   exp       is evaluated only where it decides.  With u in [2^e, 2^(e+1)) and p = 2^-t (t = d2 / sigma^2 * log2 e): t > -e means
//             p < 2^e <= u (dropped), t < -e - 1 means p > 2^(e+1) > u (kept); both with a margin of 1e-6 in t, six orders
//             above the rounding of t, so the shortcut never contradicts the predicate.  On the oracle's inputs 2 - 4 % of
//             the pairs inside the support reach exp at small sigma, a quarter when sigma spans the box.
//   geometry  optional, fill pass: the periodic builder's values (pos_src[j] - image(pos_dst[i]) on the coordinates reduced into
//             the period, and its norm, rounded once to float32) - the rows radius_csr(..., return_geometry=True) gives the edge.
namespace {

constexpr double GAUSS_LOG2E = 1.4426950408889634;
constexpr double GAUSS_Q_MAX = 37.5;                    // exp(-37.5) < 2^-54 = min u: no draw can keep the pair

struct GaussTest {
    double s2, cut2;            // sigma * sigma; cutoff^2 (+inf: no cutoff)
    uint64_t seed_term;         // seed * GPDE_HASH_SEED_MUL
};

template <bool PERIODIC>
__device__ __forceinline__ double gauss_d2(const PeriodicGrid& g, const double* __restrict__ ps, int j, const double (&xd)[3]) {
    const int dim = g.cells.dim;
    double d2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < dim) {
            const double xs = ps[(size_t)j * dim + k];
            double d;
            if (PERIODIC && g.per[k] > 0.0) {
                d = xs - xd[k];
                d = d - g.per[k] * rint(d / g.per[k]);
            } else {
                d = xd[k] - xs;
            }
            d2 += d * d;
        }
    return d2;
}

__device__ __forceinline__ bool gauss_keep(const GaussTest& gt, double d2, int i, int j) {
    if (d2 > gt.cut2) return false;
    const double q = d2 / gt.s2;
    if (!(q <= GAUSS_Q_MAX)) return false;
    uint64_t z = gt.seed_term + (((uint64_t)(uint32_t)i << 32) | (uint64_t)(uint32_t)j);
    z = (z ^ (z >> 30)) * GPDE_HASH_MUL1;
    z = (z ^ (z >> 27)) * GPDE_HASH_MUL2;
    z ^= z >> 31;
    const double u = ((double)(z >> 11) + 0.5) * 0x1p-53;              // key >> 10 = z >> 11
    const int e = (int)((__double_as_longlong(u) >> 52) & 0x7ff) - 1023;     // u in [2^e, 2^(e+1)), normal
    const double t = q * GAUSS_LOG2E;
    if (t > (double)(-e) + 1e-6) return false;
    if (t < (double)(-e - 1) - 1e-6) return true;
    return u < exp(-q);
}

template <bool PERIODIC>
__device__ __forceinline__ void gauss_geom(const PeriodicGrid& g, const double* __restrict__ ps, int j, const double (&pc)[3], float* gs) {
    const int dim = g.cells.dim;
    double d2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < dim) {
            const double x = ps[(size_t)j * dim + k];
            const double dk = (PERIODIC && g.wrap[k]) ? nearest_image_diff(reduce_into_period(x, g.cells.lo[k], g.per[k]), pc[k], g.per[k], g.half[k])
                                                      : x - pc[k];
            gs[k] = (float)dk;
            d2 += dk * dk;
        }
    gs[dim] = (float)sqrt(d2);
}

template <bool PERIODIC>
__global__ void k_gauss_cell_ids(const double* __restrict__ pos, int n, PeriodicGrid g, uint32_t* __restrict__ cell, uint32_t* __restrict__ id) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int dim = g.cells.dim;
    double p[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < dim; ++k) {
        const double x = pos[(size_t)j * dim + k];
        p[k] = PERIODIC ? reduce_into_period(x, g.cells.lo[k], g.per[k]) : x;
    }
    int c[3];
    cell_of(g.cells, p, c);
    cell[j] = (uint32_t)((c[2] * g.cells.nc[1] + c[1]) * g.cells.nc[0] + c[0]);
    id[j] = (uint32_t)j;
}

template <bool FILL, bool PERIODIC>
__global__ __launch_bounds__(256) void k_gauss_neighbors(const double* __restrict__ ps, const double* __restrict__ pd, int nd, PeriodicGrid g,
                                                         GaussTest gt, const int32_t* __restrict__ cell_start,
                                                         const uint32_t* __restrict__ order, int32_t* __restrict__ deg,
                                                         const int32_t* __restrict__ rowptr, int32_t* __restrict__ src,
                                                         int32_t* __restrict__ dst, float* __restrict__ geom, int64_t n_edges, int sort_cap) {
    extern __shared__ uint32_t sbuf[];                  // FILL: [4 waves][sort_cap], sort_cap a power of two in 64 .. CG_SORT_MAX
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * 4 + wave;
    if (i >= nd) return;
    const int dim = g.cells.dim;
    double pr[3] = {0.0, 0.0, 0.0}, pc[3] = {0.0, 0.0, 0.0};     // the destination: raw (the distance), reduced (its cell, the geometry)
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < dim) {
            pr[k] = pd[(size_t)i * dim + k];
            pc[k] = PERIODIC ? reduce_into_period(pr[k], g.cells.lo[k], g.per[k]) : pr[k];
        }
    int ci[3];
    cell_of(g.cells, pc, ci);
    const int r0 = FILL ? rowptr[i] : 0;
    const int n_row = FILL ? rowptr[i + 1] - r0 : 0;
    if (FILL && (r0 < 0 || n_row < 0 || (int64_t)r0 + n_row > n_edges)) return;      // not a rowptr of n_edges slots: nothing is written
    const bool in_lds = FILL && n_row <= sort_cap;
    const bool want_geom = FILL && geom != nullptr;
    uint32_t* row = sbuf + wave * sort_cap;
    const AxisWalk wx = axis_walk(g, 0, ci[0]), wy = axis_walk(g, 1, ci[1]), wz = axis_walk(g, 2, ci[2]);
    int count = 0;
    for (int tz = wz.a0; tz <= wz.a1 + (wz.extra >= 0 ? 1 : 0); ++tz) {
        const int cz = tz > wz.a1 ? wz.extra : tz;
        for (int ty = wy.a0; ty <= wy.a1 + (wy.extra >= 0 ? 1 : 0); ++ty) {
            const int cy = ty > wy.a1 ? wy.extra : ty;
            const int base = (cz * g.cells.nc[1] + cy) * g.cells.nc[0];
            for (int tx = 0; tx <= (wx.extra >= 0 ? 1 : 0); ++tx) {
                const int cx0 = tx ? wx.extra : wx.a0, cx1 = tx ? wx.extra : wx.a1;
                const int p0 = cell_start[base + cx0], p1 = cell_start[base + cx1 + 1];
                for (int q0 = p0; q0 < p1; q0 += 64) {
                    const int q = q0 + lane;
                    bool hit = false;
                    int j = 0;
                    if (q < p1) {
                        j = (int)order[q];
                        hit = gauss_keep(gt, gauss_d2<PERIODIC>(g, ps, j, pr), i, j);
                    }
                    const unsigned long long m = __ballot(hit);
                    if (FILL && hit) {
                        const int slot = count + __popcll(m & ((1ull << lane) - 1ull));
                        if (slot < n_row) {
                            if (in_lds) row[slot] = (uint32_t)j;
                            else {                            // very long rows: cell order (deterministic, not ascending)
                                src[r0 + slot] = j;
                                if (want_geom) gauss_geom<PERIODIC>(g, ps, j, pc, geom + (size_t)(r0 + slot) * (dim + 1));
                            }
                        }
                    }
                    count += __popcll(m);
                }
            }
        }
    }
    if (!FILL) {
        if (lane == 0) deg[i] = count;
        return;
    }
    if (in_lds) {
        sort_row_by_source(row, n_row, lane);
        for (int t = lane; t < n_row; t += 64) {
            const int j = (int)row[t];
            src[r0 + t] = j;
            if (want_geom) gauss_geom<PERIODIC>(g, ps, j, pc, geom + (size_t)(r0 + t) * (dim + 1));
        }
    }
    for (int t = lane; t < n_row; t += 64) dst[r0 + t] = i;
}

struct GaussPlan {
    PeriodicGrid g;
    GaussTest gt;
    int64_t ncells;
    bool periodic;
};

double gauss_support_radius(double sigma) { return sigma * sqrt(54.0 * 0.6931471805599453); }

// Every refusal the scalars and the host arrays show, then the grid: cells of edge >= min(r_support, cutoff).
int gauss_plan(const char* what, int dim, double sigma, double cutoff, int64_t seed, const double* lo, const double* hi,
               const double* origin, const double* period, GaussPlan* p) {
    if (dim < 1 || dim > 3) { gpde_set_error("%s: dim must be 1..3 (got %d)", what, dim); return GPDE_EUNSUPPORTED; }
    if (!(sigma > 0.0) || !isfinite(sigma) || !(sigma * sigma > 0.0) || !isfinite(sigma * sigma)) {
        gpde_set_error("%s: sigma = %g must be positive and finite (and so must sigma^2)", what, sigma);
        return GPDE_EINVAL;
    }
    if (!(cutoff >= 0.0) || !isfinite(cutoff)) { gpde_set_error("%s: cutoff = %g must be positive and finite, or 0 (none)", what, cutoff); return GPDE_EINVAL; }
    double r = gauss_support_radius(sigma);
    if (cutoff > 0.0 && cutoff < r) r = cutoff;
    if (!isfinite(r)) { gpde_set_error("%s: the support radius of sigma = %g is not finite", what, sigma); return GPDE_EINVAL; }
    p->periodic = false;
    double per[3] = {0.0, 0.0, 0.0}, org[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < dim; ++k) {
        per[k] = period ? period[k] : 0.0;
        org[k] = origin ? origin[k] : 0.0;
        if (!(per[k] >= 0.0) || !isfinite(per[k]) || !isfinite(org[k])) {
            gpde_set_error("%s: period[%d] must be >= 0 (0 = open axis) and origin[%d] finite", what, k, k);
            return GPDE_EINVAL;
        }
        if (per[k] > 0.0) {
            p->periodic = true;
            if (!(2.0 * r < per[k])) {
                gpde_set_error("%s: 2 min(r_support, cutoff) = %g >= period[%d] = %g: a pair would have more than one image in reach (pass a cutoff)",
                               what, 2.0 * r, k, per[k]);
                return GPDE_EINVAL;
            }
        }
    }
    if (int rc = make_periodic_grid(what, dim, r, lo, hi, org, per, &p->g, &p->ncells)) return rc;
    p->gt.s2 = sigma * sigma;
    p->gt.cut2 = cutoff > 0.0 ? cutoff * cutoff : INFINITY;
    p->gt.seed_term = (uint64_t)seed * GPDE_HASH_SEED_MUL;
    return GPDE_OK;
}

int gauss_check_points(const char* what, const double* ps, int64_t ns, const double* pd, int64_t nd) {
    if (ns < 0 || nd < 0 || ns > 0x7fffffff || nd > 0x7fffffff) { gpde_set_error("%s: point counts must be 0 .. 2^31 - 1", what); return GPDE_EINVAL; }
    if (!ps || !pd) { gpde_set_error("%s: pos_src / pos_dst is null", what); return GPDE_EINVAL; }
    return GPDE_OK;
}

}  // namespace

extern "C" size_t gpde_gaussian_csr_workspace_bytes(int64_t n_src, int dim, double sigma, double cutoff, const double* lo,
                                                    const double* hi, const double* origin, const double* period) {
    const char* what = "gpde_gaussian_csr_workspace_bytes";
    GaussPlan p;
    if (n_src < 0 || n_src > 0x7fffffff) { gpde_set_error("%s: n_src out of range", what); return 0; }
    if (gauss_plan(what, dim, sigma, cutoff, 0, lo, hi, origin, period, &p) != GPDE_OK) return 0;
    return carve(nullptr, n_src, p.ncells).total + 256;
}

extern "C" int gpde_gaussian_csr_count(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim, double sigma,
                                       double cutoff, int64_t seed, const double* lo, const double* hi, const double* origin,
                                       const double* period, int32_t* deg, void* ws, size_t ws_bytes, void* stream_) {
    const char* what = "gpde_gaussian_csr_count";
    hipStream_t st = (hipStream_t)stream_;
    GaussPlan p;
    if (int rc = gauss_check_points(what, pos_src, n_src, pos_dst, n_dst)) return rc;
    if (!deg || !ws) { gpde_set_error("%s: deg / ws is null", what); return GPDE_EINVAL; }
    if (int rc = gauss_plan(what, dim, sigma, cutoff, seed, lo, hi, origin, period, &p)) return rc;
    CellWs w = carve(ws, n_src, p.ncells);
    if (ws_bytes < w.total) { gpde_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, w.total); return GPDE_EWORKSPACE; }
    if (n_dst == 0) return GPDE_OK;
    const int T = 256;
    if (n_src > 0) {
        const dim3 grid((unsigned)((n_src + T - 1) / T));
        if (p.periodic) hipLaunchKernelGGL((k_gauss_cell_ids<true>), grid, dim3(T), 0, st, pos_src, (int)n_src, p.g, w.cell, w.id);
        else hipLaunchKernelGGL((k_gauss_cell_ids<false>), grid, dim3(T), 0, st, pos_src, (int)n_src, p.g, w.cell, w.id);
        GP_HIP_CHECK(rocprim::radix_sort_pairs(w.temp, w.temp_bytes, w.cell, w.cell_sorted, w.id, w.order, (size_t)n_src, 0,
                                               sort_bits_for(p.ncells), st));
    }
    hipLaunchKernelGGL(k_cell_start, dim3((unsigned)((p.ncells + 1 + T - 1) / T)), dim3(T), 0, st, w.cell_sorted, (int)n_src, (int)p.ncells, w.start);
    const dim3 grid((unsigned)((n_dst + 3) / 4)), block(256);
    if (p.periodic)
        hipLaunchKernelGGL((k_gauss_neighbors<false, true>), grid, block, 0, st, pos_src, pos_dst, (int)n_dst, p.g, p.gt, w.start, w.order, deg,
                           (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr, (int64_t)0, 0);
    else
        hipLaunchKernelGGL((k_gauss_neighbors<false, false>), grid, block, 0, st, pos_src, pos_dst, (int)n_dst, p.g, p.gt, w.start, w.order, deg,
                           (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr, (int64_t)0, 0);
    GP_LAUNCH_CHECK("gpde_gaussian_csr_count kernels");
    return GPDE_OK;
}

// `ws` must still hold what gpde_gaussian_csr_count left there (same arguments); rowptr = exclusive scan of its `deg`.
// max_in_degree (0: not known) sizes the LDS row sort: the walk waits on gathers and on float64 division, so the waves in flight
// decide its speed, and 4 rows of CG_SORT_MAX slots (64 KiB) leave two workgroups per CU where the registers would allow seven.
extern "C" int gpde_gaussian_csr_fill(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim, double sigma,
                                      double cutoff, int64_t seed, const double* lo, const double* hi, const double* origin,
                                      const double* period, const int32_t* rowptr, int32_t* src, int32_t* dst, float* geom,
                                      int64_t n_edges, int64_t max_in_degree, void* ws, size_t ws_bytes, void* stream_) {
    const char* what = "gpde_gaussian_csr_fill";
    hipStream_t st = (hipStream_t)stream_;
    GaussPlan p;
    if (int rc = gauss_check_points(what, pos_src, n_src, pos_dst, n_dst)) return rc;
    if (n_edges < 0 || n_edges > 0x7fffffff - 64) { gpde_set_error("%s: n_edges = %lld outside an int32 CSR (0 .. 2^31 - 65)", what, (long long)n_edges); return GPDE_EINVAL; }
    if (max_in_degree < 0) { gpde_set_error("%s: max_in_degree = %lld must be >= 0 (0: not known)", what, (long long)max_in_degree); return GPDE_EINVAL; }
    if (!rowptr || !ws || (n_edges > 0 && (!src || !dst))) { gpde_set_error("%s: null rowptr / src / dst / ws", what); return GPDE_EINVAL; }
    if (int rc = gauss_plan(what, dim, sigma, cutoff, seed, lo, hi, origin, period, &p)) return rc;
    CellWs w = carve(ws, n_src, p.ncells);
    if (ws_bytes < w.total) { gpde_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, w.total); return GPDE_EWORKSPACE; }
    if (n_dst == 0 || n_edges == 0) return GPDE_OK;
    const dim3 grid((unsigned)((n_dst + 3) / 4)), block(256);
    int sort_cap = CG_SORT_MAX;                          // rows up to this many edges are sorted: the smallest power of two that holds
    if (max_in_degree > 0)                               // the longest row, from one wave step (64) up to CG_SORT_MAX
        for (sort_cap = 64; sort_cap < max_in_degree && sort_cap < CG_SORT_MAX;) sort_cap <<= 1;
    const size_t lds = (size_t)4 * sort_cap * 4;
    if (p.periodic)
        hipLaunchKernelGGL((k_gauss_neighbors<true, true>), grid, block, lds, st, pos_src, pos_dst, (int)n_dst, p.g, p.gt, w.start, w.order,
                           (int32_t*)nullptr, rowptr, src, dst, geom, n_edges, sort_cap);
    else
        hipLaunchKernelGGL((k_gauss_neighbors<true, false>), grid, block, lds, st, pos_src, pos_dst, (int)n_dst, p.g, p.gt, w.start, w.order,
                           (int32_t*)nullptr, rowptr, src, dst, geom, n_edges, sort_cap);
    GP_LAUNCH_CHECK("gpde_gaussian_csr_fill kernels");
    return GPDE_OK;
}
