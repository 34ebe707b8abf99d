// Cap a graph's in-degree: per destination row of a CSR keep the k in-edges with the smallest (key, slot), and the two
// keys the host offers for it (include/gpde.h: gpde_csr_select_k, gpde_edge_keys_sqdist, gpde_edge_keys_hash).
//
// The builders of gpde_cellgraph.hip emit the FULL ball of every destination; the reference's mesh generators also offer a
// thinned connectivity next to ball_connectivity (gaussian_connectivity, graph-neural-operator utilities.py:257-263, 372-378)
// and PyG's radius_graph has max_num_neighbors.  The selection works on a finished CSR, so one kernel serves the open, periodic
// and batched builders and graphs that came from an edge_index.
//   select   one wave per destination row, four per workgroup (the sibling kernels' shape).  A row of at most k in-edges is
//            copied.  A longer row: the k-th smallest key T is found by bisection over the 64 key bits (the sign bit biased, so
//            the keys order as unsigned words) - bit by bit from the top, "how many keys are <= prefix | (all lower bits set)?",
//            counted per lane and summed over the wave - then ONE emission pass in slot order keeps key < T and the first
//            k - #{key < T} slots with key == T, placed by ballot prefix.  No sort, no atomics: the output is in ascending slot
//            order and two calls give the same bits; the selection for k is a subset of the one for any k' > k because both
//            are prefixes of the one (key, slot) order.
//   staging  rows of up to SEL_LDS_KEYS keys are read from memory once and kept in LDS (16 KiB per wave, 4 x 16 KiB per
//            workgroup like the builders' row sort); longer rows are re-read from memory on each of the 65 passes.  Lane l owns
//            the elements l, l + 64, ... in every pass, so the LDS rows are lane-private: no exchange between lanes happens
//            through LDS and no fence is needed.
//   keys     squared distance: float64, d2 += d * d in axis order with contraction off - the arithmetic of
//            k_cell_neighbors<., false>, so a float64 host computation reproduces the bits; a non-negative double orders as its
//            int64 bits; periodic axes: d = x_s - x_d, d -= L rint(d / L) on the raw coordinates (min_image_diff below).
//            Hash: the counter-based mix stated in the header.
#include "gpde_common.h"
#include <math.h>

#pragma clang fp contract(off)      // the squared-distance key is defined by where it rounds

namespace {

constexpr int SEL_LDS_KEYS = 2048;                      // keys of one row staged in LDS: 16 KiB per wave
constexpr uint64_t SEL_SIGN = 0x8000000000000000ull;    // bias of the sign bit: int64 order -> uint64 order

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <bool LDS>
__device__ __forceinline__ uint64_t sel_key(const uint64_t* row, const int64_t* __restrict__ gk, int t) {
    return LDS ? row[t] : ((uint64_t)gk[t] ^ SEL_SIGN);
}

// the row's k smallest (key, slot), emitted in slot order; n > k >= 1
template <bool LDS>
__device__ __forceinline__ void select_row(const uint64_t* row, const int64_t* __restrict__ gk, int n, int k, int r0, int64_t o0,
                                           int64_t n_out, int32_t* __restrict__ slots_out, int lane) {
    // T = the smallest word with #{u <= T} >= k
    uint64_t T = 0;
    for (int bit = 63; bit >= 0; --bit) {
        const uint64_t cand = T | ((1ull << bit) - 1ull);          // this bit 0, every lower bit 1
        int c = 0;
        for (int t = lane; t < n; t += 64) c += sel_key<LDS>(row, gk, t) <= cand ? 1 : 0;
        if (wave_sum(c) < k) T |= 1ull << bit;
    }
    int c = 0;
    for (int t = lane; t < n; t += 64) c += sel_key<LDS>(row, gk, t) < T ? 1 : 0;
    const int need = k - wave_sum(c);                                // ties at T to keep: the first `need` in slot order (>= 1)
    const unsigned long long below = (1ull << lane) - 1ull;
    int ties = 0, kept = 0;
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int t = t0 + lane;
        bool lt = false, eq = false;
        if (t < n) {
            const uint64_t u = sel_key<LDS>(row, gk, t);
            lt = u < T;
            eq = u == T;
        }
        const unsigned long long me = __ballot(eq);
        const bool keep = lt || (eq && ties + __popcll(me & below) < need);
        const unsigned long long mk = __ballot(keep);
        if (keep) {
            const int64_t o = o0 + kept + __popcll(mk & below);
            if (o >= 0 && o < n_out) slots_out[o] = r0 + t;          // (a rowptr_out that is not the scan of min(deg, k) writes nothing outside)
        }
        ties += __popcll(me);
        kept += __popcll(mk);
    }
}

__global__ __launch_bounds__(256) void k_select_k(const int32_t* __restrict__ rowptr, const int64_t* __restrict__ keys, int n_rows,
                                                  int64_t n_edges, int k, const int32_t* __restrict__ rowptr_out,
                                                  int32_t* __restrict__ slots_out, int64_t n_out) {
    extern __shared__ uint64_t sel_buf[];               // [4 waves][SEL_LDS_KEYS]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * 4 + wave;
    if (i >= n_rows) return;
    const int r0 = rowptr[i], r1 = rowptr[i + 1];
    const int64_t o0 = rowptr_out[i];
    if (r0 < 0 || r1 < r0 || r1 > n_edges) return;      // not a rowptr of n_edges slots: nothing is read
    const int n = r1 - r0;
    if (n <= k) {
        for (int t = lane; t < n; t += 64) {
            const int64_t o = o0 + t;
            if (o >= 0 && o < n_out) slots_out[o] = r0 + t;
        }
        return;
    }
    const int64_t* gk = keys + r0;
    if (n <= SEL_LDS_KEYS) {
        uint64_t* row = sel_buf + (size_t)wave * SEL_LDS_KEYS;
        for (int t = lane; t < n; t += 64) row[t] = (uint64_t)gk[t] ^ SEL_SIGN;
        select_row<true>(row, gk, n, k, r0, o0, n_out, slots_out, lane);
    } else {
        select_row<false>(nullptr, gk, n, k, r0, o0, n_out, slots_out, lane);
    }
}

struct KeyBox {
    double per[3], org[3];      // period (0: open axis) and origin per axis (checked; the difference does not depend on it)
    int dim;
};

// The minimum-image difference of a periodic axis, on the RAW coordinates: d = x_s - x_d, d -= L rint(d / L) - the textbook
// form, which a float64 host computation reproduces operation by operation (the division is correctly rounded, rint rounds
// half to even like numpy's round, contraction is off).  The periodic BUILDER reduces both points into the box and subtracts an
// image x_d +- L (gpde_cellgraph.hip); that form rounds x_d +- L at the magnitude of L, which moves the d2 of a seam-crossing
// edge by tens of ulp against the raw form (measured: up to 149 ulp inside the box) - harmless for the builder's test against
// r^2, but the key is specified to a few ulp of the host value, so it takes the form the host can follow.
__device__ __forceinline__ double min_image_diff(double xs, double xd, double L) {
    const double d = xs - xd;
    return d - L * rint(d / L);
}

__global__ void k_keys_sqdist(const double* __restrict__ ps, const double* __restrict__ pd, KeyBox b, const int32_t* __restrict__ src,
                              const int32_t* __restrict__ dst, int64_t n_edges, int64_t* __restrict__ keys) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    const int64_t j = src[e], i = dst[e];
    double d2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (a < b.dim) {
            const double xs = ps[j * b.dim + a], xd = pd[i * b.dim + a];
            double d;
            if (b.per[a] > 0.0)
                d = min_image_diff(xs, xd, b.per[a]);       // (translation-invariant: the origin does not enter)
            else
                d = xd - xs;
            d2 += d * d;
        }
    keys[e] = __double_as_longlong(d2);
}

__global__ void k_keys_hash(const int32_t* __restrict__ src_ids, const int32_t* __restrict__ dst_ids, int64_t n_edges, uint64_t seed,
                            int64_t* __restrict__ keys) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    uint64_t z = seed * GPDE_HASH_SEED_MUL + (((uint64_t)(uint32_t)dst_ids[e] << 32) | (uint64_t)(uint32_t)src_ids[e]);
    z = (z ^ (z >> 30)) * GPDE_HASH_MUL1;
    z = (z ^ (z >> 27)) * GPDE_HASH_MUL2;
    z ^= z >> 31;
    keys[e] = (int64_t)(z >> 1);
}

constexpr int64_t KEY_MAX_EDGES = (int64_t)0x7fffffff * 256;      // one thread per edge, 256 per block, 2^31 - 1 blocks

}  // namespace

extern "C" int gpde_csr_select_k(const int32_t* rowptr, const int64_t* keys, int64_t n_rows, int64_t n_edges, int64_t k,
                                 const int32_t* rowptr_out, int32_t* slots_out, int64_t n_out, void* stream_) {
    const char* what = "gpde_csr_select_k";
    hipStream_t st = (hipStream_t)stream_;
    if (k < 1) { gpde_set_error("%s: k = %lld must be >= 1", what, (long long)k); return GPDE_EINVAL; }
    if (n_rows < 0 || n_rows > 0x7fffffff || n_edges < 0 || n_edges > 0x7fffffff - 64) {      // (lanes step past a row's end by < 64)
        gpde_set_error("%s: n_rows = %lld / n_edges = %lld out of range (an int32 CSR: 0 .. 2^31 - 1 rows, 0 .. 2^31 - 65 edges)", what, (long long)n_rows, (long long)n_edges);
        return GPDE_EINVAL;
    }
    if (!rowptr || !rowptr_out) { gpde_set_error("%s: rowptr / rowptr_out is null", what); return GPDE_EINVAL; }
    if (n_edges > 0 && !keys) { gpde_set_error("%s: keys is null", what); return GPDE_EINVAL; }
    // rowptr_out lives on the device and the call never synchronises: what the host sees of its total is the range it can lie in
    // (the kernel writes no slot at or past n_out whatever rowptr_out holds)
    const int64_t most = n_rows == 0 ? 0 : (k >= n_edges ? n_edges : (n_rows > n_edges / k ? n_edges : n_rows * k));
    if (n_out < 0 || n_out > most) {
        gpde_set_error("%s: n_out = %lld is not the total of rowptr_out (the scan of min(deg, k)): at most %lld for %lld rows, %lld edges, k = %lld",
                       what, (long long)n_out, (long long)most, (long long)n_rows, (long long)n_edges, (long long)k);
        return GPDE_EINVAL;
    }
    if (n_edges > 0 && n_rows == 0) { gpde_set_error("%s: %lld edges in a graph without rows", what, (long long)n_edges); return GPDE_EINVAL; }
    if (n_out > 0 && !slots_out) { gpde_set_error("%s: slots_out is null", what); return GPDE_EINVAL; }
    if (n_rows == 0 || n_edges == 0 || n_out == 0) return GPDE_OK;
    const int kk = (int)(k > 0x7fffffff ? 0x7fffffff : k);
    hipLaunchKernelGGL(k_select_k, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), (size_t)4 * SEL_LDS_KEYS * sizeof(uint64_t), st, rowptr, keys,
                       (int)n_rows, n_edges, kk, rowptr_out, slots_out, n_out);
    GP_LAUNCH_CHECK("gpde_csr_select_k kernel");
    return GPDE_OK;
}

extern "C" int gpde_edge_keys_sqdist(const double* pos_src, const double* pos_dst, int dim, const double* period, const double* origin,
                                     const int32_t* src, const int32_t* dst, int64_t n_edges, int64_t* keys, void* stream_) {
    const char* what = "gpde_edge_keys_sqdist";
    hipStream_t st = (hipStream_t)stream_;
    if (dim < 1 || dim > 3) { gpde_set_error("%s: dim must be 1..3 (got %d)", what, dim); return GPDE_EUNSUPPORTED; }
    if (n_edges < 0 || n_edges > KEY_MAX_EDGES) { gpde_set_error("%s: n_edges = %lld out of range", what, (long long)n_edges); return GPDE_EINVAL; }
    KeyBox b{};
    b.dim = dim;
    for (int a = 0; a < dim; ++a) {
        b.per[a] = period ? period[a] : 0.0;
        b.org[a] = origin ? origin[a] : 0.0;
        if (!(b.per[a] >= 0.0) || !isfinite(b.per[a]) || !isfinite(b.org[a])) {
            gpde_set_error("%s: period[%d] must be >= 0 (0 = open axis) and origin[%d] finite", what, a, a);
            return GPDE_EINVAL;
        }
    }
    if (n_edges > 0 && (!pos_src || !pos_dst || !src || !dst || !keys)) {
        gpde_set_error("%s: pos_src / pos_dst / src / dst / keys is null", what);
        return GPDE_EINVAL;
    }
    if (n_edges == 0) return GPDE_OK;
    hipLaunchKernelGGL(k_keys_sqdist, dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, st, pos_src, pos_dst, b, src, dst, n_edges, keys);
    GP_LAUNCH_CHECK("gpde_edge_keys_sqdist kernel");
    return GPDE_OK;
}

extern "C" int gpde_edge_keys_hash(const int32_t* src_ids, const int32_t* dst_ids, int64_t n_edges, int64_t seed, int64_t* keys,
                                   void* stream_) {
    const char* what = "gpde_edge_keys_hash";
    hipStream_t st = (hipStream_t)stream_;
    if (n_edges < 0 || n_edges > KEY_MAX_EDGES) { gpde_set_error("%s: n_edges = %lld out of range", what, (long long)n_edges); return GPDE_EINVAL; }
    if (n_edges > 0 && (!src_ids || !dst_ids || !keys)) { gpde_set_error("%s: src_ids / dst_ids / keys is null", what); return GPDE_EINVAL; }
    if (n_edges == 0) return GPDE_OK;
    hipLaunchKernelGGL(k_keys_hash, dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, st, src_ids, dst_ids, n_edges, (uint64_t)seed, keys);
    GP_LAUNCH_CHECK("gpde_edge_keys_hash kernel");
    return GPDE_OK;
}
