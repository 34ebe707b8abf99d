// Exact k-nearest-neighbour graph, emitted directly as the destination-sorted CSR the operator consumes: gpde_knn_csr
// (include/gpde.h states the contract; DESIGN.md §6e "The nearest arm").
//
// Row i holds the k_eff sources j of smallest (d2_bits(j, i), j): d2 the float64 squared distance in the arithmetic of
// gpde_edge_keys_sqdist (open axes), ties to the smaller source id - what gpde_csr_select_k keeps of the complete bipartite
// graph under those keys.  Every row has k_eff edges, so rowptr[i] = i k_eff is known before anything runs: one pass, no count,
// no scan, no synchronisation.
//   setup     the sources are binned into cubic cells of edge h by the cell list of gpde_cellgraph.hip (gpde_cells.h);
//   search    one wave per DESTINATION walks the Chebyshev rings rho = 0, 1, 2, ... of cells around its own cell.  The rows of a
//             ring (fixed cy, cz) are spread over the lanes, each looks up its one or two ranges of the sorted list (the whole
//             x-range on the faces of the ring, its two end cells elsewhere) and the wave then visits the non-empty ranges, 64
//             candidates per step.  A candidate that sorts before the current k-th pair is appended to the wave's LDS buffer of
//             CAP = 2 KP pairs (KP = the power of two >= max(k, 64)); when fewer than 64 slots are free the buffer is bitonic-sorted
//             by (key, src) and cut back to the k best, whose last pair is the new filter;
//   stop      after ring rho, once k pairs are held: stop iff the k-th d2 is BELOW a lower bound of every key an unvisited cell
//             can hold (an equal key of smaller id must still win its tie).  An unvisited cell differs from the centre by more
//             than rho on some axis a; a source binned there has floor((x - lo) inv) >= c + rho + 1 (or <= c - rho - 1) in the
//             binning's own arithmetic, hence x >= lo + (c + rho + 1) h (1 - 4u), u = 2^-53.  The bound takes the face
//             lo + (c + rho + 1) h as computed, minus the destination coordinate, minus a slack of 2^-48 (|lo| + |x_d| + (nc + 1) h)
//             - 32 u of every magnitude that enters, against the 8 u the roundings of binning, face and key can add up to - clamps
//             at 0, squares and scales by (1 - 2^-50).  Sides without cells (the border cells are unbounded outward: they hold
//             the clamped points) give no term; the bound never uses the destination's own cell, so it holds for a destination
//             outside the box as well;
//   loops     the ring loop is a `for` to the host-given largest grid extent; ranges are clipped to [0, n_src]; a NaN compares
//             false everywhere it could extend a loop or move an index;
//   emit      the k ids are sorted ascending in LDS (the row sort of the other builders), src / dst and the optional geometry
//             row (pos[src] - pos_dst[dst] and its norm, float64 rounded once: the open radius builder's values) are written.
// No atomics; the result does not depend on h, on the launch geometry or on the order in which candidates arrive: the buffer
// is a set, cut by a total order.
#include "gpde_cells.h"
#include <float.h>
#include <math.h>

#pragma clang fp contract(off)      // the key is defined by where it rounds

// The automatic cell edge: the mean occupancy of a cell is m = max(2, k / 2) sources, so that the k nearest of a destination in a
// uniform cloud lie within about one ring.  The cloud's dimension is taken from its box: with the extents sorted descending,
// h = max over d' = 1 .. dim of (m e_1 .. e_d' / n_src)^(1 / d') - a flat or line-like box gets the spacing of the axes that
// have extent, not a fine grid across the thin ones.  A box without extent: h = 1 (one cell).
double knn_auto_cell(int dim, int64_t n_src, int k, const double* lo, const double* hi) {
    double e[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < dim; ++a) e[a] = hi[a] - lo[a];
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (e[b] > e[a]) { const double t = e[a]; e[a] = e[b]; e[b] = t; }
    const double m = k / 2 > 2 ? (double)(k / 2) : 2.0, n = n_src > 0 ? (double)n_src : 1.0;
    double h = 0.0, prod = 1.0;
    for (int d = 1; d <= dim; ++d) {
        prod *= e[d - 1];
        const double c = pow(m * prod / n, 1.0 / d);
        if (c > h && isfinite(c)) h = c;
    }
    return h > 0.0 && isfinite(1.0 / h) ? h : 1.0;
}

namespace {

struct KnnGrid {
    CellGrid cells;
    double h;                   // cell edge; cells.inv = 1 / h
    double mag[3];              // |lo| + (nc + 1) h per axis: the slack of the stopping rule, before the destination's share
};

__global__ __launch_bounds__(256) void k_knn_rowptr(int32_t* __restrict__ rowptr, int n_dst, int k_eff) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n_dst) rowptr[i] = (int32_t)(i * k_eff);
}

__global__ __launch_bounds__(256) void k_knn_search(const double* __restrict__ ps, int ns, const double* __restrict__ pd, int nd, KnnGrid g,
                                                    int k, int skip_self, int n_rings, int cap,
                                                    const int32_t* __restrict__ cell_start, const uint32_t* __restrict__ order,
                                                    int32_t* __restrict__ src, int32_t* __restrict__ dst, float* __restrict__ geom) {
    extern __shared__ int64_t knn_lds[];                 // [4 waves][cap] keys, then [4 waves][cap] ids
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * 4 + wave;
    if (i >= nd) return;
    int64_t* key = knn_lds + wave * cap;
    uint32_t* id = (uint32_t*)(knn_lds + 4 * cap) + wave * cap;
    const int dim = g.cells.dim;
    double xd[3] = {0.0, 0.0, 0.0}, slack[3] = {0.0, 0.0, 0.0};
    int ci[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (a < dim) {
            xd[a] = pd[(size_t)i * dim + a];
            slack[a] = 0x1p-48 * (g.mag[a] + fabs(xd[a]));
            // the centre of the walk: cell_of's value for every finite coordinate; the comparisons are on the double, so a NaN
            // lands in cell 0 like anything else that is not >= 0
            const double t = floor((xd[a] - g.cells.lo[a]) * g.cells.inv[a]);
            ci[a] = !(t >= 0.0) ? 0 : (t >= (double)g.cells.nc[a] ? g.cells.nc[a] - 1 : (int)t);
        }
    const int nx = g.cells.nc[0], ny = g.cells.nc[1], nz = g.cells.nc[2];
    int rmax = 0;                                       // the ring that reaches the farthest border
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (a < dim) rmax = max(rmax, max(ci[a], g.cells.nc[a] - 1 - ci[a]));
    rmax = min(rmax, n_rings - 1);

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
        const int y0 = dim > 1 ? max(-rho, -ci[1]) : 0, y1 = dim > 1 ? min(rho, ny - 1 - ci[1]) : 0;
        const int z0 = dim > 2 ? max(-rho, -ci[2]) : 0, z1 = dim > 2 ? min(rho, nz - 1 - ci[2]) : 0;
        const int wy = y1 - y0 + 1, rows = wy * (z1 - z0 + 1);
        const int xl = ci[0] - rho, xr = ci[0] + rho;
        for (int t0 = 0; t0 < rows; t0 += 64) {
            const int t = t0 + lane;
            int rng[2][2] = {{0, 0}, {0, 0}};           // this lane's row: up to two ranges of the sorted list
            if (t < rows) {
                const int dy = y0 + t % wy, dz = z0 + t / wy;
                const int base = ((ci[2] + dz) * ny + (ci[1] + dy)) * nx;
                if (max(abs(dy), abs(dz)) == rho) {     // a face of the ring: its whole x-range is contiguous in the list
                    rng[0][0] = cell_start[base + max(xl, 0)];
                    rng[0][1] = cell_start[base + min(xr, nx - 1) + 1];
                } else {                                // inside: the two end cells (rho > 0 here)
                    if (xl >= 0) { rng[0][0] = cell_start[base + xl]; rng[0][1] = cell_start[base + xl + 1]; }
                    if (xr <= nx - 1) { rng[1][0] = cell_start[base + xr]; rng[1][1] = cell_start[base + xr + 1]; }
                }
            }
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                const int r0 = max(rng[part][0], 0), r1 = min(rng[part][1], ns);
                unsigned long long m = __ballot(r1 > r0);
                const int n_ranges = __popcll(m);
                for (int b = 0; b < n_ranges; ++b) {
                    const int owner = __ffsll((long long)m) - 1;
                    m &= m - 1ull;
                    const int p0 = __shfl(r0, owner), p1 = __shfl(r1, owner);
                    for (int q0 = p0; q0 < p1; q0 += 64) {
                        if (cnt > cap - 64) compact();  // room for a whole step (cap - k >= 64)
                        const int q = q0 + lane;
                        bool hit = false;
                        int j = 0;
                        int64_t kb = 0;
                        if (q < p1) {
                            j = (int)order[q];
                            if ((unsigned)j < (unsigned)ns && !(skip_self && j == i)) {
                                double d2 = 0.0;
#pragma unroll
                                for (int a = 0; a < 3; ++a)
                                    if (a < dim) {
                                        const double d = xd[a] - ps[(size_t)j * dim + a];
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
                    if (cp <= g.cells.nc[a] - 1) {
                        const double gap = ((g.cells.lo[a] + (double)cp * g.h) - xd[a]) - slack[a];
                        gmin = fmin(gmin, gap > 0.0 ? gap : 0.0);            // (a NaN gap counts as 0: go on)
                    }
                    if (cm >= 0) {
                        const double gap = (xd[a] - (g.cells.lo[a] + (double)(cm + 1) * g.h)) - slack[a];
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
    const size_t r0 = (size_t)i * k;
    for (int t = lane; t < k; t += 64) {
        int j = t < n_found ? (int)id[t] : 0;
        if ((unsigned)j >= (unsigned)ns) j = 0;
        src[r0 + t] = j;
        dst[r0 + t] = i;
        if (geom != nullptr) {
            float* gs = geom + (r0 + t) * (dim + 1);
            double d2 = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (a < dim) {
                    const double da = ps[(size_t)j * dim + a] - xd[a];
                    gs[a] = (float)da;
                    d2 += da * da;
                }
            gs[dim] = (float)sqrt(d2);
        }
    }
}

struct KnnPlan {
    KnnGrid g;
    int64_t ncells;
    int n_rings;                // the grid's largest extent in cells
    int k_eff;
    int skip_self;
    int cap;                    // pairs per wave in LDS
};

// Every refusal the scalars and the host arrays show, then the grid.
int knn_plan(const char* what, int64_t n_src, int64_t n_dst, int dim, int64_t k, int loop, int same_set, double cell, const double* lo,
             const double* hi, KnnPlan* p) {
    if (dim < 1 || dim > 3) { gpde_set_error("%s: dim must be 1..3 (got %d)", what, dim); return GPDE_EUNSUPPORTED; }
    if (k < 1 || k > GPDE_KNN_MAX_K) { gpde_set_error("%s: k = %lld must be 1 .. %d (GPDE_KNN_MAX_K)", what, (long long)k, GPDE_KNN_MAX_K); return GPDE_EINVAL; }
    if (loop != 0 && loop != 1) { gpde_set_error("%s: loop = %d must be 0 or 1", what, loop); return GPDE_EINVAL; }
    if (n_src < 0 || n_dst < 0 || n_src > 0x7fffffff || n_dst > 0x7fffffff) { gpde_set_error("%s: point counts must be 0 .. 2^31 - 1", what); return GPDE_EINVAL; }
    if (!(cell >= 0.0) || !isfinite(cell) || (cell > 0.0 && !isfinite(1.0 / cell))) {
        gpde_set_error("%s: cell = %g must be 0 (automatic) or a positive finite edge with a finite reciprocal", what, cell);
        return GPDE_EINVAL;
    }
    if (!lo || !hi) { gpde_set_error("%s: host bounds lo / hi required", what); return GPDE_EINVAL; }
    for (int a = 0; a < dim; ++a)
        if (!isfinite(lo[a]) || !isfinite(hi[a]) || !(hi[a] >= lo[a]) || !isfinite(hi[a] - lo[a])) {
            gpde_set_error("%s: the box [%g, %g] in dimension %d is empty or not finite", what, lo[a], hi[a], a);
            return GPDE_EINVAL;
        }
    p->skip_self = same_set && !loop;
    const int64_t have = n_src - (p->skip_self ? 1 : 0);
    p->k_eff = (int)(k < have ? k : (have > 0 ? have : 0));
    if ((int64_t)p->k_eff * n_dst > 0x7fffffff - 64) {
        gpde_set_error("%s: n_dst * k_eff = %lld edges outside an int32 CSR (0 .. 2^31 - 65)", what, (long long)p->k_eff * (long long)n_dst);
        return GPDE_EINVAL;
    }
    int kp = 64;
    while (kp < p->k_eff) kp <<= 1;
    p->cap = 2 * kp;
    double h = cell > 0.0 ? cell : knn_auto_cell(dim, n_src, (int)k, lo, hi);
    for (;; h *= 2.0) {                                 // too many cells: coarser ones (the result does not depend on h)
        int64_t tot = 1;
        bool fits = isfinite(h);
        p->n_rings = 1;
        for (int a = 0; a < 3; ++a) {
            p->g.cells.lo[a] = 0.0; p->g.cells.inv[a] = 0.0; p->g.cells.nc[a] = 1; p->g.mag[a] = 0.0;
            if (a >= dim) continue;
            const double cells = floor((hi[a] - lo[a]) / h) + 1.0;
            if (!(cells <= (double)KNN_NC_MAX)) { fits = false; continue; }
            const int nc = cells < 1.0 ? 1 : (int)cells;
            p->g.cells.lo[a] = lo[a]; p->g.cells.inv[a] = 1.0 / h; p->g.cells.nc[a] = nc;
            p->g.mag[a] = fabs(lo[a]) + ((double)nc + 1.0) * h;
            if (nc > p->n_rings) p->n_rings = nc;
            tot *= nc;
        }
        if (!isfinite(h)) { gpde_set_error("%s: no finite cell edge covers the box", what); return GPDE_EINVAL; }
        if (fits && tot <= KNN_CELLS_MAX) { p->ncells = tot; break; }
    }
    p->g.cells.dim = dim;
    p->g.h = h;
    return GPDE_OK;
}

}  // namespace

extern "C" size_t gpde_knn_csr_workspace_bytes(int64_t n_src, int64_t n_dst, int dim, int64_t k, double cell, const double* lo,
                                               const double* hi) {
    KnnPlan p;
    if (knn_plan("gpde_knn_csr_workspace_bytes", n_src, n_dst, dim, k, 1, 0, cell, lo, hi, &p) != GPDE_OK) return 0;
    return gpde_cell_list_ws_bytes(n_src, p.ncells);
}

extern "C" int gpde_knn_csr(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim, int64_t k, int loop,
                            double cell, const double* lo, const double* hi, int32_t* rowptr, int32_t* src, int32_t* dst, float* geom,
                            void* ws, size_t ws_bytes, void* stream_) {
    const char* what = "gpde_knn_csr";
    hipStream_t st = (hipStream_t)stream_;
    KnnPlan p;
    const int same = pos_src == pos_dst && n_src == n_dst;
    if (int rc = knn_plan(what, n_src, n_dst, dim, k, loop, same, cell, lo, hi, &p)) return rc;
    if ((n_src > 0 && !pos_src) || (n_dst > 0 && !pos_dst)) { gpde_set_error("%s: pos_src / pos_dst is null", what); return GPDE_EINVAL; }
    const int64_t n_edges = (int64_t)p.k_eff * n_dst;
    if (!rowptr || !ws || (n_edges > 0 && (!src || !dst))) { gpde_set_error("%s: null rowptr / src / dst / ws", what); return GPDE_EINVAL; }
    const size_t need = gpde_cell_list_ws_bytes(n_src, p.ncells) - 256;
    if (ws_bytes < need) { gpde_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, need); return GPDE_EWORKSPACE; }
    hipLaunchKernelGGL(k_knn_rowptr, dim3((unsigned)((n_dst + 1 + 255) / 256)), dim3(256), 0, st, rowptr, (int)n_dst, p.k_eff);
    if (n_edges > 0) {
        GpdeCellList cl;
        if (int rc = gpde_cell_list_build(what, pos_src, n_src, p.g.cells, p.ncells, ws, ws_bytes, st, &cl)) return rc;
        const size_t lds = (size_t)4 * p.cap * (sizeof(int64_t) + sizeof(uint32_t));
        hipLaunchKernelGGL(k_knn_search, dim3((unsigned)((n_dst + 3) / 4)), dim3(256), lds, st, pos_src, (int)n_src, pos_dst, (int)n_dst, p.g,
                           p.k_eff, p.skip_self, p.n_rings, p.cap, cl.start, cl.order, src, dst, geom);
    }
    GP_LAUNCH_CHECK("gpde_knn_csr kernels");
    return GPDE_OK;
}
