// The two further arms of the exact k-nearest-neighbour builder (gpde_knn.hip is the open one): gpde_knn_csr_batched - the kNN
// graphs of B point sets in one build - and gpde_knn_csr_periodic - the kNN graph on a torus
// (include/gpde.h states the contracts; DESIGN.md §6e "The batched nearest arm", "The periodic nearest arm").
//
// Both run ONE search kernel, k_knn_search_arms: the open arm's - one wave per destination, Chebyshev rings of cells, the k best
// (key, source) pairs in an LDS buffer cut by a bitonic sort, the same stopping rule - generalised in three places:
//   view      what a wave needs of its grid (KnnView) is a kernel argument on the torus and is read from the record of the
//             destination's graph in a batch: the graph's own grid, its first cell in the batch-wide numbering, its source range,
//             its k_eff and its first CSR slot.  The wave finds the record by a scalar binary search over the records' dst_end;
//   rings     every axis has a range of cell OFFSETS [omin, omax] around the centre cell c: [-c, nc - 1 - c] on an open axis (the
//             open arm's clipping), [-(nc - 1) / 2, nc / 2] on a periodic one - nc consecutive offsets, which wrapped modulo nc
//             name every cell of the axis exactly once.  Ring rho visits the offset vectors of Chebyshev norm rho inside these
//             ranges, so a cell is visited once however few cells an axis has (nc = 1: offset 0 only; nc = 2: 0 and +1; nc = 3:
//             -1 .. 1).  The x-range of a face row, wrapped, is at most two contiguous ranges of the sorted list;
//   key       on a periodic axis d = x_src - x_dst, d -= L rint(d / L) on the RAW coordinates (gpde_edge_keys_sqdist), on an open
//             one x_dst - x_src as in the open arm; squares summed in axis order, contraction off.
// The torus bins REDUCED coordinates (x - L floor((x - origin) / L), the destination's likewise) while the key is taken from the
// raw ones.  The stopping rule therefore argues on the circle: after ring rho with 2 rho + 1 < nc cells of a periodic axis
// visited, every unvisited cell of that axis lies on the arc from the face origin + (c + rho + 1) h up to the face
// origin + (c - rho) h + L, so the minimum-image distance of its points from the reduced destination x is at least
// min(face_plus - x, x - face_minus); an axis whose nc cells are all visited gives no term.  What separates the computed
// quantities from the real ones - the reduction of source and destination (4 u of |x| + |origin| + L each), the binning product,
// the faces, and the raw key's own rounding (3 u of |x_src| + |x_dst| + L) - is below 16 u of
// M = max_j |x_src[j]| + |x_dst| + |origin| + 2 L, and the bound subtracts 2^-46 M = 128 u M.  max_j |x_src[j]| is reduced on the device
// by the binning pass (per-block maxima, then one block; no host read-back): a point 2^20 periods outside the box widens the
// slack, which only makes the walk go further.  `>=` continues, so an unvisited equal key of smaller id still wins its tie.
// No atomics, no synchronisation, no allocation; the buffer is a set cut by a total order, so the result does not depend on the
// grid, the origin or the order in which candidates arrive.
#include "gpde_cells.h"
#include <float.h>
#include <math.h>

#pragma clang fp contract(off)      // the key is defined by where it rounds

namespace {

struct KnnView {
    double lo[3], inv[3], h[3];     // per axis: the grid's anchor, cells per unit length, cell edge
    double per[3];                  // period; 0: an open axis
    double mag[3];                  // the slack's magnitude before the destination's share (and the sources' maximum on the torus)
    int nc[3];
    int cell_base, k, skip_self, n_rings;
};

struct KnnBatchRec {
    double lo[3], inv[3];
    double h;
    double mag[3];
    int32_t nc[3];
    int32_t cell_base;
    int32_t src_begin, src_end, dst_begin, dst_end;
    int32_t k_eff, edge_base, n_rings, pad;
};
static_assert(sizeof(KnnBatchRec) == GPDE_KNN_BATCHED_REC_BYTES, "KnnBatchRec is the record of include/gpde.h");

// the graph that owns point `p`: the first record whose range ends after p (empty graphs in between are passed over)
template <bool DST>
__device__ __forceinline__ int knn_graph_of(const KnnBatchRec* __restrict__ tab, int n_graphs, int p) {
    int lo = 0, hi = n_graphs - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((DST ? tab[mid].dst_end : tab[mid].src_end) <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// rowptr of both arms: tab == nullptr: i k_eff; a batch: the row's first slot from its graph's record, rowptr[n_dst] = n_edges
__global__ __launch_bounds__(256) void k_knn_rowptr_arms(int32_t* __restrict__ rowptr, int n_dst, int k_eff, const KnnBatchRec* __restrict__ tab,
                                                         int n_graphs, int n_edges) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_dst) return;
    if (tab == nullptr) { rowptr[i] = (int32_t)(i * k_eff); return; }
    if (i == n_dst) { rowptr[i] = n_edges; return; }
    const KnnBatchRec& t = tab[knn_graph_of<true>(tab, n_graphs, (int)i)];
    rowptr[i] = t.edge_base + ((int)i - t.dst_begin) * t.k_eff;
}

__global__ void k_knn_cell_ids_batched(const double* __restrict__ pos, int n, int dim, const KnnBatchRec* __restrict__ tab, int n_graphs,
                                       uint32_t* __restrict__ cell, uint32_t* __restrict__ id) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const KnnBatchRec& t = tab[knn_graph_of<false>(tab, n_graphs, j)];
    CellGrid g;
#pragma unroll
    for (int a = 0; a < 3; ++a) { g.lo[a] = t.lo[a]; g.inv[a] = t.inv[a]; g.nc[a] = t.nc[a]; }
    g.dim = dim;
    double p[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < dim; ++a) p[a] = pos[(size_t)j * dim + a];
    int c[3];
    cell_of(g, p, c);
    cell[j] = (uint32_t)(t.cell_base + (c[2] * g.nc[1] + c[1]) * g.nc[0] + c[0]);
    id[j] = (uint32_t)j;
}

__device__ __forceinline__ double knn_reduce(double x, double o, double L) { return L > 0.0 ? x - L * floor((x - o) / L) : x; }

// max over 256 threads of three values each, left in sm[a][0]
__device__ __forceinline__ void block_max3(double (&sm)[3][256], const double (&m)[3]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int a = 0; a < 3; ++a) sm[a][t] = m[a];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int a = 0; a < 3; ++a) sm[a][t] = fmax(sm[a][t], sm[a][t + s]);
        __syncthreads();
    }
}

// the torus: sources binned by their reduced coordinates; block_max[block][a] = the block's largest |raw coordinate|
__global__ __launch_bounds__(256) void k_knn_cell_ids_periodic(const double* __restrict__ pos, int n, int dim, KnnView v, uint32_t* __restrict__ cell,
                                                               uint32_t* __restrict__ id, double* __restrict__ block_max) {
    __shared__ double sm[3][256];
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    double m[3] = {0.0, 0.0, 0.0};
    if (j < n) {
        CellGrid g;
#pragma unroll
        for (int a = 0; a < 3; ++a) { g.lo[a] = v.lo[a]; g.inv[a] = v.inv[a]; g.nc[a] = v.nc[a]; }
        g.dim = dim;
        double p[3] = {0.0, 0.0, 0.0};
        for (int a = 0; a < dim; ++a) {
            const double x = pos[(size_t)j * dim + a];
            m[a] = fabs(x);
            p[a] = knn_reduce(x, v.lo[a], v.per[a]);
        }
        int c[3];
        cell_of(g, p, c);
        cell[j] = (uint32_t)((c[2] * g.nc[1] + c[1]) * g.nc[0] + c[0]);
        id[j] = (uint32_t)j;
    }
    block_max3(sm, m);
    if (threadIdx.x < 3) block_max[(size_t)blockIdx.x * 3 + threadIdx.x] = sm[threadIdx.x][0];
}

__global__ __launch_bounds__(256) void k_knn_src_mag(const double* __restrict__ block_max, int n_blocks, double* __restrict__ src_mag) {
    __shared__ double sm[3][256];
    double m[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < n_blocks; b += 256)
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] = fmax(m[a], block_max[(size_t)b * 3 + a]);
    block_max3(sm, m);
    if (threadIdx.x < 3) src_mag[threadIdx.x] = sm[threadIdx.x][0];
}

__device__ __forceinline__ int wrap_cell(int c, int nc) { return c < 0 ? c + nc : (c >= nc ? c - nc : c); }

template <bool BATCHED>
__global__ __launch_bounds__(256) void k_knn_search_arms(const double* __restrict__ ps, int ns, const double* __restrict__ pd, int nd, int dim,
                                                         KnnView pv, const KnnBatchRec* __restrict__ tab, int n_graphs,
                                                         const double* __restrict__ src_mag, int cap,
                                                         const int32_t* __restrict__ cell_start, const uint32_t* __restrict__ order,
                                                         int32_t* __restrict__ src, int32_t* __restrict__ dst, float* __restrict__ geom) {
    extern __shared__ int64_t knn_arms_lds[];            // [4 waves][cap] keys, then [4 waves][cap] ids
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * 4 + wave;
    if (i >= nd) return;
    int64_t* key = knn_arms_lds + wave * cap;
    uint32_t* id = (uint32_t*)(knn_arms_lds + 4 * cap) + wave * cap;
    KnnView v = pv;
    int src_lo = 0, src_hi = ns;                        // the ids a candidate may have
    size_t r0;
    if (BATCHED) {
        const KnnBatchRec& t = tab[knn_graph_of<true>(tab, n_graphs, i)];
        if (i < t.dst_begin || i >= t.dst_end || t.k_eff <= 0) return;          // (a graph without usable sources: empty rows)
#pragma unroll
        for (int a = 0; a < 3; ++a) { v.lo[a] = t.lo[a]; v.inv[a] = t.inv[a]; v.h[a] = t.h; v.mag[a] = t.mag[a]; v.nc[a] = t.nc[a]; }
        v.cell_base = t.cell_base; v.k = t.k_eff; v.n_rings = t.n_rings;
        src_lo = max(t.src_begin, 0); src_hi = min(t.src_end, ns);
        r0 = (size_t)t.edge_base + (size_t)(i - t.dst_begin) * t.k_eff;
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (a < dim) v.mag[a] += src_mag[a];
        r0 = (size_t)i * v.k;
    }
    const int k = v.k, skip_self = v.skip_self;
    double xd[3] = {0.0, 0.0, 0.0}, xr[3] = {0.0, 0.0, 0.0}, slack[3] = {0.0, 0.0, 0.0};
    int ci[3] = {0, 0, 0}, omin[3] = {0, 0, 0}, omax[3] = {0, 0, 0};
    int rmax = 0;                                       // the ring that reaches the farthest offset
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (a < dim) {
            xd[a] = pd[(size_t)i * dim + a];
            xr[a] = knn_reduce(xd[a], v.lo[a], v.per[a]);
            slack[a] = 0x1p-46 * (v.mag[a] + fabs(xd[a]));
            // the comparisons are on the double, so a NaN lands in cell 0 like anything else that is not >= 0
            const double t = floor((xr[a] - v.lo[a]) * v.inv[a]);
            ci[a] = !(t >= 0.0) ? 0 : (t >= (double)v.nc[a] ? v.nc[a] - 1 : (int)t);
            if (v.per[a] > 0.0) { omin[a] = -((v.nc[a] - 1) / 2); omax[a] = v.nc[a] / 2; }
            else { omin[a] = -ci[a]; omax[a] = v.nc[a] - 1 - ci[a]; }
            rmax = max(rmax, max(-omin[a], omax[a]));
        }
    rmax = min(rmax, v.n_rings - 1);
    const int nx = v.nc[0], ny = v.nc[1], nz = v.nc[2];

    int cnt = 0;                                        // pairs in the buffer (wave-uniform)
    bool have = false;                                  // the buffer was cut to k: (thr_key, thr_id) is its k-th pair
    int64_t thr_key = 0;
    uint32_t thr_id = 0;
    auto compact = [&]() {                              // sort what is held; keep the k best
        int np2 = 64;
        while (np2 < cnt) np2 <<= 1;                    // cnt <= cap, a power of two
        for (int t = cnt + lane; t < np2; t += 64) { key[t] = INT64_MAX; id[t] = 0xffffffffu; }
        sort_pairs(key, id, np2, lane);
        if (cnt >= k) {
            cnt = k;
            have = true;
            thr_key = key[k - 1];
            thr_id = id[k - 1];
        }
    };

    for (int rho = 0; rho <= rmax; ++rho) {
        const int y0 = max(-rho, omin[1]), y1 = min(rho, omax[1]);
        const int z0 = max(-rho, omin[2]), z1 = min(rho, omax[2]);
        const int wy = y1 - y0 + 1, rows = wy * (z1 - z0 + 1);
        const int xa = ci[0] + max(-rho, omin[0]), xb = ci[0] + min(rho, omax[0]);      // the face rows' x-range, unwrapped: xa <= ci <= xb
        for (int t0 = 0; t0 < rows; t0 += 64) {
            const int t = t0 + lane;
            int rng[2][2] = {{0, 0}, {0, 0}};           // this lane's row: up to two ranges of the sorted list
            if (t < rows) {
                const int dy = y0 + t % wy, dz = z0 + t / wy;
                const int base = v.cell_base + (wrap_cell(ci[2] + dz, nz) * ny + wrap_cell(ci[1] + dy, ny)) * nx;
                int c[2][2] = {{0, -1}, {0, -1}};       // first and last cell of each part (empty: last < first)
                if (max(abs(dy), abs(dz)) == rho) {     // a face of the ring: its x-range, in two parts where it crosses the seam
                    if (xa < 0) { c[0][0] = xa + nx; c[0][1] = nx - 1; c[1][0] = 0; c[1][1] = xb; }
                    else if (xb > nx - 1) { c[0][0] = xa; c[0][1] = nx - 1; c[1][0] = 0; c[1][1] = xb - nx; }
                    else { c[0][0] = xa; c[0][1] = xb; }
                } else {                                // inside: the two end cells (rho > 0 here)
                    if (-rho >= omin[0]) c[0][0] = c[0][1] = wrap_cell(ci[0] - rho, nx);
                    if (rho <= omax[0]) c[1][0] = c[1][1] = wrap_cell(ci[0] + rho, nx);
                }
#pragma unroll
                for (int part = 0; part < 2; ++part)
                    if (c[part][1] >= c[part][0] && c[part][0] >= 0 && c[part][1] <= nx - 1) {
                        rng[part][0] = cell_start[base + c[part][0]];
                        rng[part][1] = cell_start[base + c[part][1] + 1];
                    }
            }
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                const int q_lo = max(rng[part][0], 0), q_hi = min(rng[part][1], ns);
                unsigned long long m = __ballot(q_hi > q_lo);
                const int n_ranges = __popcll(m);
                for (int b = 0; b < n_ranges; ++b) {
                    const int owner = __ffsll((long long)m) - 1;
                    m &= m - 1ull;
                    const int p0 = __shfl(q_lo, owner), p1 = __shfl(q_hi, owner);
                    for (int q0 = p0; q0 < p1; q0 += 64) {
                        if (cnt > cap - 64) compact();  // room for a whole step (cap - k >= 64)
                        const int q = q0 + lane;
                        bool hit = false;
                        int j = 0;
                        int64_t kb = 0;
                        if (q < p1) {
                            j = (int)order[q];
                            if (j >= src_lo && j < src_hi && !(skip_self && j == i)) {
                                double d2 = 0.0;
#pragma unroll
                                for (int a = 0; a < 3; ++a)
                                    if (a < dim) {
                                        const double xs = ps[(size_t)j * dim + a];
                                        double d;
                                        if (v.per[a] > 0.0) {
                                            d = xs - xd[a];
                                            d = d - v.per[a] * rint(d / v.per[a]);
                                        } else {
                                            d = xd[a] - xs;
                                        }
                                        d2 += d * d;
                                    }
                                kb = __double_as_longlong(d2);
                                hit = !have || kb < thr_key || (kb == thr_key && (uint32_t)j < thr_id);
                            }
                        }
                        const unsigned long long mh = __ballot(hit);
                        if (hit) {
                            const int slot = cnt + __popcll(mh & ((1ull << lane) - 1ull));
                            key[slot] = kb;
                            id[slot] = (uint32_t)j;
                        }
                        cnt += __popcll(mh);
                    }
                }
            }
        }
        if (cnt >= k) {
            if (cnt > k || !have) compact();
            double gmin = INFINITY;                     // the nearest face behind which unvisited cells lie
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (a < dim) {
                    const int cp = ci[a] + rho + 1, cm = ci[a] - rho - 1;
                    const bool periodic = v.per[a] > 0.0;
                    const bool more = 2 * rho + 1 < v.nc[a];                   // a periodic axis: cells beyond the ring, on both sides
                    if (periodic ? more : cp <= v.nc[a] - 1) {
                        const double gap = ((v.lo[a] + (double)cp * v.h[a]) - xr[a]) - slack[a];
                        gmin = fmin(gmin, gap > 0.0 ? gap : 0.0);            // (a NaN gap counts as 0: go on)
                    }
                    if (periodic ? more : cm >= 0) {
                        const double gap = (xr[a] - (v.lo[a] + (double)(cm + 1) * v.h[a])) - slack[a];
                        gmin = fmin(gmin, gap > 0.0 ? gap : 0.0);
                    }
                }
            const double bound = gmin * gmin * (1.0 - 0x1p-50);
            if (__longlong_as_double(thr_key) < bound) break;
        }
    }
    if (cnt > k || (cnt == k && !have)) compact();
    const int n_found = min(cnt, k);                    // k whenever the ring loop covered the grid (k_eff <= the candidates there are)
    wave_lds_fence();
    sort_row_by_source(id, n_found, lane);
    for (int t = lane; t < k; t += 64) {
        int j = t < n_found ? (int)id[t] : src_lo;
        if (j < src_lo || j >= src_hi) j = src_lo;
        src[r0 + t] = j;
        dst[r0 + t] = i;
        if (geom != nullptr) {
            float* gs = geom + (r0 + t) * (dim + 1);
            double d2 = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (a < dim) {
                    double da = ps[(size_t)j * dim + a] - xd[a];
                    if (v.per[a] > 0.0) da = da - v.per[a] * rint(da / v.per[a]);
                    gs[a] = (float)da;
                    d2 += da * da;
                }
            gs[dim] = (float)sqrt(d2);
        }
    }
}

// ---- host: what both arms check alike ----------------------------------------------------------------------------------------------
int check_scalars(const char* what, int dim, int64_t k, int loop, double cell) {
    if (dim < 1 || dim > 3) { gpde_set_error("%s: dim must be 1..3 (got %d)", what, dim); return GPDE_EUNSUPPORTED; }
    if (k < 1 || k > GPDE_KNN_MAX_K) { gpde_set_error("%s: k = %lld must be 1 .. %d (GPDE_KNN_MAX_K)", what, (long long)k, GPDE_KNN_MAX_K); return GPDE_EINVAL; }
    if (loop != 0 && loop != 1) { gpde_set_error("%s: loop = %d must be 0 or 1", what, loop); return GPDE_EINVAL; }
    if (!(cell >= 0.0) || !isfinite(cell) || (cell > 0.0 && !isfinite(1.0 / cell))) {
        gpde_set_error("%s: cell = %g must be 0 (automatic) or a positive finite edge with a finite reciprocal", what, cell);
        return GPDE_EINVAL;
    }
    return GPDE_OK;
}

bool box_ok(double lo, double hi) { return isfinite(lo) && isfinite(hi) && hi >= lo && isfinite(hi - lo); }

int64_t k_eff_of(int64_t k, int64_t n_src, int skip_self) {
    const int64_t have = n_src - (skip_self ? 1 : 0);
    return k < have ? k : (have > 0 ? have : 0);
}

int lds_cap(int64_t k_eff) {                            // pairs per wave in LDS: twice the power of two >= max(k_eff, 64)
    int kp = 64;
    while (kp < k_eff) kp <<= 1;
    return 2 * kp;
}

size_t al256(size_t v) { return (v + 255) / 256 * 256; }

// the arms' own buffers lie behind the cell list's part of the workspace
char* behind_cell_list(void* ws, int64_t n_src, int64_t ncells) {
    return (char*)(((uintptr_t)ws + gpde_cell_list_ws_bytes(n_src, ncells) + 255) / 256 * 256);
}

// ---- the torus -------------------------------------------------------------------------------------------------------------------
struct PeriodicPlan {
    KnnView v;
    int64_t ncells;
    int cap;
    int64_t mag_blocks;         // blocks of the binning pass: [mag_blocks][3] maxima, then the 3 reduced ones
    size_t ws_bytes;
};

int periodic_plan(const char* what, int64_t n_src, int64_t n_dst, int dim, int64_t k, int loop, int same_set, double cell, const double* lo,
                  const double* hi, const double* origin, const double* period, PeriodicPlan* p) {
    if (int rc = check_scalars(what, dim, k, loop, cell)) return rc;
    if (n_src < 0 || n_dst < 0 || n_src > 0x7fffffff || n_dst > 0x7fffffff) { gpde_set_error("%s: point counts must be 0 .. 2^31 - 1", what); return GPDE_EINVAL; }
    if (!period) { gpde_set_error("%s: host array period[dim] required (0: an open axis)", what); return GPDE_EINVAL; }
    double blo[3] = {0.0, 0.0, 0.0}, bhi[3] = {0.0, 0.0, 0.0};              // the box of the grid: the period, or lo / hi on an open axis
    for (int a = 0; a < dim; ++a) {
        const double L = period[a], o = origin ? origin[a] : 0.0;
        if (!(L >= 0.0) || !isfinite(L)) { gpde_set_error("%s: period[%d] = %g must be finite and >= 0 (0: an open axis)", what, a, L); return GPDE_EINVAL; }
        if (!isfinite(o)) { gpde_set_error("%s: origin[%d] = %g must be finite", what, a, o); return GPDE_EINVAL; }
        if (L > 0.0) {
            if (!isfinite(1.0 / L) || !isfinite(o + L)) { gpde_set_error("%s: period[%d] = %g has no finite reciprocal or origin + period is not finite", what, a, L); return GPDE_EINVAL; }
            blo[a] = o; bhi[a] = o + L;
        } else {
            if (!lo || !hi) { gpde_set_error("%s: host bounds lo / hi required (axis %d is open)", what, a); return GPDE_EINVAL; }
            if (!box_ok(lo[a], hi[a])) { gpde_set_error("%s: the box [%g, %g] in dimension %d is empty or not finite", what, lo[a], hi[a], a); return GPDE_EINVAL; }
            blo[a] = lo[a]; bhi[a] = hi[a];
        }
    }
    KnnView& v = p->v;
    v.skip_self = same_set && !loop;
    v.k = (int)k_eff_of(k, n_src, v.skip_self);
    if ((int64_t)v.k * n_dst > 0x7fffffff - 64) {
        gpde_set_error("%s: n_dst * k_eff = %lld edges outside an int32 CSR (0 .. 2^31 - 65)", what, (long long)v.k * (long long)n_dst);
        return GPDE_EINVAL;
    }
    p->cap = lds_cap(v.k);
    v.cell_base = 0;
    double h = cell > 0.0 ? cell : knn_auto_cell(dim, n_src, (int)k, blo, bhi);
    for (;; h *= 2.0) {                                 // too many cells: coarser ones (the result does not depend on h)
        if (!isfinite(h)) { gpde_set_error("%s: no finite cell edge covers the box", what); return GPDE_EINVAL; }
        int64_t tot = 1;
        bool fits = true;
        v.n_rings = 1;
        for (int a = 0; a < 3; ++a) {
            v.lo[a] = 0.0; v.inv[a] = 0.0; v.h[a] = 1.0; v.per[a] = 0.0; v.mag[a] = 0.0; v.nc[a] = 1;
            if (a >= dim) continue;
            const double L = period[a];
            // a periodic axis is tiled exactly: nc = floor(L / h) cells of edge L / nc >= h (a cell edge of L / 3 gives 3 cells,
            // whatever the division rounds to)
            const double cells = L > 0.0 ? floor(L / h * (1.0 + 0x1p-30)) : floor((bhi[a] - blo[a]) / h) + 1.0;
            if (!(cells <= (double)KNN_NC_MAX)) { fits = false; continue; }
            const int nc = cells < 1.0 ? 1 : (int)cells;
            v.lo[a] = blo[a]; v.nc[a] = nc; v.per[a] = L;
            v.h[a] = L > 0.0 ? L / nc : h;
            v.inv[a] = L > 0.0 ? nc / L : 1.0 / h;
            if (!isfinite(v.inv[a])) { gpde_set_error("%s: the cells of axis %d have no finite reciprocal edge", what, a); return GPDE_EINVAL; }
            v.mag[a] = fabs(blo[a]) + 2.0 * ((double)nc + 1.0) * v.h[a];
            if (nc > v.n_rings) v.n_rings = nc;
            tot *= nc;
        }
        if (fits && tot <= KNN_CELLS_MAX) { p->ncells = tot; break; }
    }
    p->mag_blocks = (n_src + 255) / 256;
    p->ws_bytes = gpde_cell_list_ws_bytes(n_src, p->ncells) + 256 + al256((size_t)(p->mag_blocks + 1) * 3 * sizeof(double));
    return GPDE_OK;
}

}  // namespace

extern "C" size_t gpde_knn_csr_periodic_workspace_bytes(int64_t n_src, int64_t n_dst, int dim, int64_t k, double cell, const double* lo,
                                                        const double* hi, const double* origin, const double* period) {
    PeriodicPlan p;
    if (periodic_plan("gpde_knn_csr_periodic_workspace_bytes", n_src, n_dst, dim, k, 1, 0, cell, lo, hi, origin, period, &p) != GPDE_OK) return 0;
    return p.ws_bytes;
}

extern "C" int gpde_knn_csr_periodic(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim, int64_t k, int loop,
                                     double cell, const double* lo, const double* hi, const double* origin, const double* period,
                                     int32_t* rowptr, int32_t* src, int32_t* dst, float* geom, void* ws, size_t ws_bytes, void* stream_) {
    const char* what = "gpde_knn_csr_periodic";
    hipStream_t st = (hipStream_t)stream_;
    PeriodicPlan p;
    const int same = pos_src == pos_dst && n_src == n_dst;
    if (int rc = periodic_plan(what, n_src, n_dst, dim, k, loop, same, cell, lo, hi, origin, period, &p)) return rc;
    if ((n_src > 0 && !pos_src) || (n_dst > 0 && !pos_dst)) { gpde_set_error("%s: pos_src / pos_dst is null", what); return GPDE_EINVAL; }
    const int64_t n_edges = (int64_t)p.v.k * n_dst;
    if (!rowptr || !ws || (n_edges > 0 && (!src || !dst))) { gpde_set_error("%s: null rowptr / src / dst / ws", what); return GPDE_EINVAL; }
    if (ws_bytes < p.ws_bytes) { gpde_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, p.ws_bytes); return GPDE_EWORKSPACE; }
    hipLaunchKernelGGL(k_knn_rowptr_arms, dim3((unsigned)((n_dst + 1 + 255) / 256)), dim3(256), 0, st, rowptr, (int)n_dst, p.v.k,
                       (const KnnBatchRec*)nullptr, 0, (int)n_edges);
    if (n_edges > 0) {
        GpdeCellSlots s;
        GpdeCellList cl;
        const size_t cl_bytes = gpde_cell_list_ws_bytes(n_src, p.ncells);
        if (int rc = gpde_cell_list_slots(what, n_src, p.ncells, ws, cl_bytes, &s)) return rc;
        double* block_max = (double*)behind_cell_list(ws, n_src, p.ncells);
        double* src_mag = block_max + (size_t)p.mag_blocks * 3;
        hipLaunchKernelGGL(k_knn_cell_ids_periodic, dim3((unsigned)p.mag_blocks), dim3(256), 0, st, pos_src, (int)n_src, dim, p.v, s.cell, s.id, block_max);
        hipLaunchKernelGGL(k_knn_src_mag, dim3(1), dim3(256), 0, st, block_max, (int)p.mag_blocks, src_mag);
        if (int rc = gpde_cell_list_finish(what, n_src, p.ncells, ws, cl_bytes, st, &cl)) return rc;
        const size_t lds = (size_t)4 * p.cap * (sizeof(int64_t) + sizeof(uint32_t));
        hipLaunchKernelGGL((k_knn_search_arms<false>), dim3((unsigned)((n_dst + 3) / 4)), dim3(256), lds, st, pos_src, (int)n_src, pos_dst, (int)n_dst, dim,
                           p.v, (const KnnBatchRec*)nullptr, 0, src_mag, p.cap, cl.start, cl.order, src, dst, geom);
    }
    GP_LAUNCH_CHECK("gpde_knn_csr_periodic kernels");
    return GPDE_OK;
}

// ---- the batch -------------------------------------------------------------------------------------------------------------------
namespace {

// what the plan and the call both derive from the host arrays: every refusal they show, E and the largest k_eff
int batch_shape(const char* what, const int64_t* ptr_src, const int64_t* ptr_dst, int64_t n_graphs, int dim, int64_t k, int loop, double cell,
                int64_t n_src, int64_t n_dst, int64_t* n_edges, int64_t* k_max) {
    if (int rc = check_scalars(what, dim, k, loop, cell)) return rc;
    if (n_graphs < 0 || n_graphs > 0x7ffffffe) { gpde_set_error("%s: n_graphs = %lld out of range (0 .. 2^31 - 2)", what, (long long)n_graphs); return GPDE_EINVAL; }
    if (int rc = gpde_batch_check_ptr(what, "ptr_src", ptr_src, n_graphs, n_src)) return rc;
    if (int rc = gpde_batch_check_ptr(what, "ptr_dst", ptr_dst, n_graphs, n_dst)) return rc;
    int64_t e = 0, km = 0;
    for (int64_t b = 0; b < n_graphs; ++b) {
        const int64_t ke = k_eff_of(k, ptr_src[b + 1] - ptr_src[b], !loop);
        e += ke * (ptr_dst[b + 1] - ptr_dst[b]);
        if (ke > km) km = ke;
        if (e > 0x7fffffff - 64) { gpde_set_error("%s: the sum of nd_b * k_eff[b] passes %lld edges at graph %lld: outside an int32 CSR (0 .. 2^31 - 65)", what, (long long)e, (long long)b); return GPDE_EINVAL; }
    }
    *n_edges = e;
    *k_max = km;
    return GPDE_OK;
}

}  // namespace

// HOST ONLY.  bounds [B][2][dim] (lo then hi of graph b; not read for a graph without sources), ptr_src / ptr_dst [B + 1]
// (ptr_dst NULL: one point set).  table (nullable: a query) receives B records.
extern "C" int gpde_knn_csr_batched_plan(const double* bounds, const int64_t* ptr_src, const int64_t* ptr_dst, int64_t n_graphs, int dim,
                                         int64_t k, int loop, double cell, void* table, int64_t* n_cells, size_t* ws_bytes, int64_t* n_edges) {
    const char* what = "gpde_knn_csr_batched_plan";
    if (!n_cells || !ws_bytes || !n_edges) { gpde_set_error("%s: n_cells / ws_bytes / n_edges is null", what); return GPDE_EINVAL; }
    if (!ptr_dst) ptr_dst = ptr_src;
    int64_t e = 0, k_max = 0;
    if (int rc = batch_shape(what, ptr_src, ptr_dst, n_graphs, dim, k, loop, cell, -1, -1, &e, &k_max)) return rc;
    if (n_graphs > 0 && !bounds) { gpde_set_error("%s: host array bounds[n_graphs][2][dim] required", what); return GPDE_EINVAL; }
    for (int64_t b = 0; b < n_graphs; ++b) {
        if (ptr_src[b + 1] == ptr_src[b]) continue;
        const double *lo = bounds + (size_t)b * 2 * dim, *hi = lo + dim;
        for (int a = 0; a < dim; ++a)
            if (!box_ok(lo[a], hi[a])) {
                gpde_set_error("%s: the box [%g, %g] of graph %lld in dimension %d is empty or not finite", what, lo[a], hi[a], (long long)b, a);
                return GPDE_EINVAL;
            }
    }
    KnnBatchRec* tab = (KnnBatchRec*)table;
    int64_t total = 0;
    for (double scale = 1.0;; scale *= 2.0) {              // over the cap: every graph's cell edge doubles (the result does not depend on it)
        total = 0;
        bool fits = true;
        int64_t edge_base = 0;
        for (int64_t b = 0; b < n_graphs; ++b) {
            const int64_t ns_b = ptr_src[b + 1] - ptr_src[b];
            KnnBatchRec t{};
            t.h = 1.0;
            t.n_rings = 1;
            int64_t cells_b = 1;
            for (int a = 0; a < 3; ++a) t.nc[a] = 1;
            if (ns_b > 0) {                                // (no sources: one empty cell, whatever the bounds hold)
                const double *lo = bounds + (size_t)b * 2 * dim, *hi = lo + dim;
                const double h = (cell > 0.0 ? cell : knn_auto_cell(dim, ns_b, (int)k, lo, hi)) * scale;
                t.h = h;
                for (int a = 0; a < dim; ++a) {
                    const double cells = isfinite(h) ? floor((hi[a] - lo[a]) / h) + 1.0 : 1.0;
                    if (!(cells <= (double)KNN_NC_MAX)) { fits = false; continue; }
                    const int nc = cells < 1.0 ? 1 : (int)cells;
                    t.lo[a] = lo[a]; t.inv[a] = isfinite(h) ? 1.0 / h : 0.0; t.nc[a] = nc;
                    t.mag[a] = fabs(lo[a]) + 2.0 * ((double)nc + 1.0) * h;
                    if (nc > t.n_rings) t.n_rings = nc;
                    cells_b *= nc;
                }
            }
            t.cell_base = (int32_t)total;
            t.src_begin = (int32_t)ptr_src[b]; t.src_end = (int32_t)ptr_src[b + 1];
            t.dst_begin = (int32_t)ptr_dst[b]; t.dst_end = (int32_t)ptr_dst[b + 1];
            t.k_eff = (int32_t)k_eff_of(k, ns_b, !loop);
            t.edge_base = (int32_t)edge_base;
            edge_base += (int64_t)t.k_eff * (ptr_dst[b + 1] - ptr_dst[b]);
            if (tab) tab[b] = t;
            total += cells_b;
            if (!fits || (total > KNN_CELLS_MAX && total > n_graphs)) break;      // coarsen every graph and start over
        }
        if (fits && (total <= KNN_CELLS_MAX || total <= n_graphs)) break;         // one cell per graph cannot be coarsened further
    }
    *n_cells = total;
    *ws_bytes = gpde_cell_list_ws_bytes(ptr_src[n_graphs], total);
    *n_edges = e;
    return GPDE_OK;
}

extern "C" int gpde_knn_csr_batched(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim, int64_t k, int loop,
                                    const int64_t* ptr_src, const int64_t* ptr_dst, int64_t n_graphs, const void* table, int64_t n_cells,
                                    int32_t* rowptr, int32_t* src, int32_t* dst, float* geom, int64_t n_edges, void* ws, size_t ws_bytes,
                                    void* stream_) {
    const char* what = "gpde_knn_csr_batched";
    hipStream_t st = (hipStream_t)stream_;
    if (n_src < 0 || n_dst < 0 || n_src > 0x7fffffff || n_dst > 0x7fffffff) { gpde_set_error("%s: point counts must be 0 .. 2^31 - 1", what); return GPDE_EINVAL; }
    if (!ptr_dst) ptr_dst = ptr_src;
    int64_t e = 0, k_max = 0;
    if (int rc = batch_shape(what, ptr_src, ptr_dst, n_graphs, dim, k, loop, 0.0, n_src, n_dst, &e, &k_max)) return rc;
    const int same = pos_src == pos_dst && n_src == n_dst;
    if (same)                                              // ONE point set: one division into graphs
        for (int64_t b = 0; b <= n_graphs; ++b)
            if (ptr_dst[b] != ptr_src[b]) {
                gpde_set_error("%s: pos_dst is pos_src (one point set) but ptr_dst[%lld] = %lld differs from ptr_src[%lld] = %lld", what,
                               (long long)b, (long long)ptr_dst[b], (long long)b, (long long)ptr_src[b]);
                return GPDE_EINVAL;
            }
    if (!same && !loop) { gpde_set_error("%s: loop = 0 excludes the pairs of equal id, which only one point set has: two point sets pass loop = 1", what); return GPDE_EINVAL; }
    if ((n_src > 0 && !pos_src) || (n_dst > 0 && !pos_dst)) { gpde_set_error("%s: pos_src / pos_dst is null", what); return GPDE_EINVAL; }
    if (n_edges != e) { gpde_set_error("%s: n_edges = %lld, the ptr arrays give %lld", what, (long long)n_edges, (long long)e); return GPDE_EINVAL; }
    if (n_graphs > 0 && !table) { gpde_set_error("%s: the device table of gpde_knn_csr_batched_plan is null", what); return GPDE_EINVAL; }
    if (n_cells < n_graphs || n_cells > 0x7ffffffe) { gpde_set_error("%s: n_cells = %lld is not what the plan returned for %lld graphs", what, (long long)n_cells, (long long)n_graphs); return GPDE_EINVAL; }
    if (!rowptr || !ws || (e > 0 && (!src || !dst))) { gpde_set_error("%s: null rowptr / src / dst / ws", what); return GPDE_EINVAL; }
    const size_t need = gpde_cell_list_ws_bytes(n_src, n_cells) - 256;
    if (ws_bytes < need) { gpde_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, need); return GPDE_EWORKSPACE; }
    const KnnBatchRec* tab = (const KnnBatchRec*)table;
    hipLaunchKernelGGL(k_knn_rowptr_arms, dim3((unsigned)((n_dst + 1 + 255) / 256)), dim3(256), 0, st, rowptr, (int)n_dst, 0, n_graphs > 0 ? tab : nullptr,
                       (int)n_graphs, (int)e);
    if (e > 0) {
        GpdeCellSlots s;
        GpdeCellList cl;
        if (int rc = gpde_cell_list_slots(what, n_src, n_cells, ws, ws_bytes, &s)) return rc;
        hipLaunchKernelGGL(k_knn_cell_ids_batched, dim3((unsigned)((n_src + 255) / 256)), dim3(256), 0, st, pos_src, (int)n_src, dim, tab, (int)n_graphs, s.cell, s.id);
        if (int rc = gpde_cell_list_finish(what, n_src, n_cells, ws, ws_bytes, st, &cl)) return rc;
        const int cap = lds_cap(k_max);
        const size_t lds = (size_t)4 * cap * (sizeof(int64_t) + sizeof(uint32_t));
        KnnView v{};
        v.skip_self = !loop;
        hipLaunchKernelGGL((k_knn_search_arms<true>), dim3((unsigned)((n_dst + 3) / 4)), dim3(256), lds, st, pos_src, (int)n_src, pos_dst, (int)n_dst, dim,
                           v, tab, (int)n_graphs, (const double*)nullptr, cap, cl.start, cl.order, src, dst, geom);
    }
    GP_LAUNCH_CHECK("gpde_knn_csr_batched kernels");
    return GPDE_OK;
}
