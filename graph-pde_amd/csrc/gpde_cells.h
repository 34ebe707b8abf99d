// The uniform cell list of the graph builders, shared between gpde_cellgraph.hip (radius, periodic, batched and sampled graphs)
// and gpde_knn.hip (k nearest neighbours): the grid record, the binning arithmetic, the wave's LDS row sort, and the host call
// that bins one source set (cell ids -> stable radix sort by cell -> first position of every cell).
#pragma once
#include "gpde_common.h"
#include <math.h>

struct CellGrid {
    double lo[3], inv[3];
    int nc[3];
    int dim;
};

__device__ __forceinline__ void cell_of(const CellGrid& g, const double* p, int (&c)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[k] = 0;
        if (k < g.dim) {
            int v = (int)floor((p[k] - g.lo[k]) * g.inv[k]);
            c[k] = v < 0 ? 0 : (v >= g.nc[k] ? g.nc[k] - 1 : v);
        }
    }
}

// One wave's row in LDS, sorted by source id (distinct keys): bitonic, padded with sentinels to a power of two.
__device__ __forceinline__ void sort_row_by_source(uint32_t* row, int n_row, int lane) {
    int np2 = 64;
    while (np2 < n_row) np2 <<= 1;
    for (int t = n_row + lane; t < np2; t += 64) row[t] = 0xffffffffu;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // LDS operations of one wave execute in order: a
    __builtin_amdgcn_wave_barrier();                             // compiler fence is all the exchange between lanes needs
    for (int k = 2; k <= np2; k <<= 1)
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int t = lane; t < np2; t += 64) {
                const int p = t ^ jj;
                if (p > t) {
                    const uint32_t a = row[t], b = row[p];
                    const bool up = (t & k) == 0;
                    if ((a > b) == up) { row[t] = b; row[p] = a; }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
}

// One wave's exchange through LDS: its LDS operations execute in order, a compiler fence is all the lanes need between them.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ascending bitonic sort of np2 (a power of two >= 64) pairs by (key, id): the k-best buffer of the nearest-neighbour arms
__device__ __forceinline__ void sort_pairs(int64_t* key, uint32_t* id, int np2, int lane) {
    wave_lds_fence();
    for (int k = 2; k <= np2; k <<= 1)
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int t = lane; t < np2; t += 64) {
                const int p = t ^ jj;
                if (p > t) {
                    const int64_t ka = key[t], kb = key[p];
                    const uint32_t ia = id[t], ib = id[p];
                    const bool up = (t & k) == 0;
                    const bool a_after_b = ka > kb || (ka == kb && ia > ib);
                    if (a_after_b == up) { key[t] = kb; key[p] = ka; id[t] = ib; id[p] = ia; }
                }
            }
            wave_lds_fence();
        }
}

// What the nearest-neighbour arms (gpde_knn.hip, gpde_knn_arms.hip) share on the host: the limits of a grid and the automatic
// cell edge (defined in gpde_knn.hip).
constexpr int KNN_NC_MAX = 1 << 16;                     // cells per axis: bounds the ring loop
constexpr int64_t KNN_CELLS_MAX = (int64_t)1 << 24;     // cells in all (the cap of the other builders)
double knn_auto_cell(int dim, int64_t n_src, int k, const double* lo, const double* hi);

// The cell list of `n_src` points in grid `g` (ncells = nc[0] nc[1] nc[2] <= 2^24), built on `st` inside `ws`
// (gpde_cell_list_ws_bytes; no allocation, no synchronisation): the members of cell c = (cz nc[1] + cy) nc[0] + cx are
// order[start[c] .. start[c + 1]), ascending point id inside a cell.  Defined in gpde_cellgraph.hip.
struct GpdeCellList {
    const int32_t* start;       // [ncells + 1]
    const uint32_t* order;      // [n_src]
};
size_t gpde_cell_list_ws_bytes(int64_t n_src, int64_t ncells);
int gpde_cell_list_build(const char* what, const double* pos_src, int64_t n_src, const CellGrid& g, int64_t ncells, void* ws,
                         size_t ws_bytes, hipStream_t st, GpdeCellList* out);
// The same in two steps, for a caller that bins by a rule of its own (a batch's per-graph grids, reduced periodic
// coordinates): _slots carves `ws` and hands out cell[n_src] / id[n_src] for the caller's kernel to fill on `st` (id[j] = j);
// _finish sorts them by cell and writes the first position of every cell.
struct GpdeCellSlots { uint32_t* cell; uint32_t* id; };
int gpde_cell_list_slots(const char* what, int64_t n_src, int64_t ncells, void* ws, size_t ws_bytes, GpdeCellSlots* out);
int gpde_cell_list_finish(const char* what, int64_t n_src, int64_t ncells, void* ws, size_t ws_bytes, hipStream_t st, GpdeCellList* out);
// ptr[0] = 0 <= ptr[1] <= ... <= ptr[B] = n <= 2^31 - 1 (n < 0: the end is not compared): the rule of every batched builder
int gpde_batch_check_ptr(const char* what, const char* name, const int64_t* ptr, int64_t n_graphs, int64_t n);
