// GCNConv (Kipf & Welling) on a destination CSR: the baseline every table of the multipole paper compares the kernel networks
// against (multipole-graph-neural-operator/neurips4_GCN.py: `GCNConv(width, width)` 16 times per forward on the 421^2 grid).
//
//   gpde_gcn_norm   PyG's gcn_norm with add_remaining_self_loops: per CSR slot coef_e = dinv[src] w_e dinv[dst], per node
//                   self_coef_i = dinv[i]^2 * (self weight); the degree is the TARGET-side sum (PyG >= 1.6).
//   gpde_gcn_fwd    out[i] = (sum_{e -> i} coef_e x[src_e] + self_coef_i x[i]) . W + bias: aggregate FIRST, multiply by W while
//                   the aggregated tile is still in LDS - one [N][C] round trip less than SpMM followed by a GEMM.
//
// One workgroup (4 waves) owns GCN_TM = 64 destination rows.  Phase 1: each wave aggregates 16 of them, lanes across channels
// (channel = lane + 64 p), so a gathered source row is one coalesced read per pass; src / coef of 64 in-edges are loaded by the
// lanes at once and broadcast.  A row is summed two-level: chains of at most 64 in-edges, the chain sums added in order - the
// error of a row of thousands of edges grows with length / 64 + 64 instead of its length.  The fp32 rows go to an
// LDS tile [64][kstride], kstride = 2 mod 64: the MFMA's A reads (32 rows x 2 k) then hit 64 different banks.
// Phase 2: tile . W on v_mfma_f32_32x32x2_f32 (exact fp32, an fmaf chain over k), W read from L2 (at most 256 KiB, shared by
// every workgroup); wave w owns the 32-column blocks w, w + 4.  Epilogue: bias, optional ReLU, one store.
// No atomics: one writer per output element and a summation order fixed by the graph - two calls give the same bits.
#include "gpde_common.h"

namespace {

constexpr int GCN_TM = 64;        // destination rows per workgroup (two MFMA row blocks)
constexpr int GCN_MAXW = GPDE_WECONV_ANY_MAX_WIDTH;

static inline int gcn_kstride(int cin) { return (cin + 61) / 64 * 64 + 2; }       // >= cin rounded up to even, = 2 mod 64

struct GcnArgs {
    const float* x; const int32_t* rowptr; const int32_t* src; const float* coef; const float* self_coef;
    const float* W; const float* bias; float* out; float* agg_out;
    int n_nodes, cin, cout, relu, kstride;
};

// ---- normalisation -------------------------------------------------------------------------------------------------------------
// one thread per destination row, slots in ascending order, float64 accumulation: deg (and with it dinv) is a function of the
// graph alone.  selfw[i]: the weight of the node's self loop (an existing self-loop edge of largest original id, else `fill`).
__global__ __launch_bounds__(256) void k_gcn_degree(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                                                    const int32_t* __restrict__ perm, const float* __restrict__ ew, int n,
                                                    int self_loops, float fill, double* __restrict__ dinv, float* __restrict__ selfw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int e0 = rowptr[i], e1 = rowptr[i + 1];
    double deg = 0.0;
    float sw = fill;
    int best = -1;
    for (int s = e0; s < e1; ++s) {
        const int id = perm ? perm[s] : s;
        const float w = ew ? ew[id] : 1.f;
        if (self_loops && src[s] == i) {
            if (id > best) { best = id; sw = w; }
        } else {
            deg += (double)w;
        }
    }
    if (self_loops) deg += (double)sw;
    dinv[i] = deg > 0.0 ? 1.0 / sqrt(deg) : 0.0;
    selfw[i] = sw;
}

// one wave per destination row, lanes across its slots
__global__ __launch_bounds__(256) void k_gcn_coef(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                                                  const int32_t* __restrict__ perm, const float* __restrict__ ew, int n,
                                                  int self_loops, int normalize, const double* __restrict__ dinv,
                                                  const float* __restrict__ selfw, float* __restrict__ coef, float* __restrict__ self_coef) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int e0 = rowptr[i], e1 = rowptr[i + 1];
    const double di = normalize ? dinv[i] : 0.0;
    for (int s = e0 + lane; s < e1; s += 64) {
        const float w = ew ? ew[perm ? perm[s] : s] : 1.f;
        const int j = src[s];
        float c = w;
        if (normalize) c = (self_loops && j == i) ? 0.f : (float)(dinv[j] * (double)w * di);
        coef[s] = c;
    }
    if (lane == 0) self_coef[i] = (normalize && self_loops) ? (float)(di * di * (double)selfw[i]) : 0.f;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <int NP>
__device__ __forceinline__ void gcn_aggregate_row(const GcnArgs& a, int i, int lane, float (&tot)[NP]) {
#pragma unroll
    for (int p = 0; p < NP; ++p) tot[p] = 0.f;
    const int e0 = a.rowptr[i], e1 = a.rowptr[i + 1];
    for (int b = e0; b < e1; b += 64) {
        const int nb = min(64, e1 - b);
        int js = 0;
        float cs = 0.f;
        if (lane < nb) {
            js = a.src[b + lane];
            cs = a.coef[b + lane];
            if ((unsigned)js >= (unsigned)a.n_nodes) { js = 0; cs = 0.f; }      // (a CSR of the library has none: never read outside x)
        }
        float part[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) part[p] = 0.f;
#pragma unroll 4
        for (int t = 0; t < nb; ++t) {
            const int j = __shfl(js, t);
            const float c = __shfl(cs, t);
            const float* xr = a.x + (size_t)j * a.cin;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int ch = lane + 64 * p;
                if (ch < a.cin) part[p] = fmaf(c, xr[ch], part[p]);
            }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) tot[p] += part[p];
    }
    if (a.self_coef) {
        const float sc = a.self_coef[i];
        const float* xr = a.x + (size_t)i * a.cin;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int ch = lane + 64 * p;
            if (ch < a.cin) tot[p] = fmaf(sc, xr[ch], tot[p]);
        }
    }
}

template <int NP, bool HASW>
__global__ __launch_bounds__(256) void gpde_gcn_fwd_kernel(GcnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gcn_tile[];      // [GCN_TM][kstride] (HASW only)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * GCN_TM;
    const int ks = a.kstride;
    for (int r = wave; r < GCN_TM; r += 4) {
        const int i = r0 + r;
        float tot[NP];
        if (i < a.n_nodes) {
            gcn_aggregate_row<NP>(a, i, lane, tot);
        } else {
#pragma unroll
            for (int p = 0; p < NP; ++p) tot[p] = 0.f;
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int ch = lane + 64 * p;
            if (ch >= a.cin) continue;
            if (HASW) gcn_tile[r * ks + ch] = tot[p];
            if (i < a.n_nodes) {
                if (a.agg_out) a.agg_out[(size_t)i * a.cin + ch] = tot[p];
                if (!HASW) {
                    float v = tot[p] + (a.bias ? a.bias[ch] : 0.f);
                    if (a.relu) v = fmaxf(v, 0.f);
                    a.out[(size_t)i * a.cin + ch] = v;
                }
            }
        }
        if (HASW && (a.cin & 1) && lane == 0) gcn_tile[r * ks + a.cin] = 0.f;      // the K tail: the MFMA steps over k in pairs
    }
    if (!HASW) return;
    __syncthreads();
    const int l31 = lane & 31, h = lane >> 5;
    const int ncb = (a.cout + 31) / 32;
    const float* t0 = gcn_tile + l31 * ks + h;
    const float* t1 = t0 + 32 * ks;
    for (int cb = wave; cb < ncb; cb += 4) {
        const int col = cb * 32 + l31;
        const bool colok = col < a.cout;
        const float* wp = a.W + (colok ? col : 0);
        f32x16 acc0, acc1;
#pragma unroll
        for (int j = 0; j < 16; ++j) { acc0[j] = 0.f; acc1[j] = 0.f; }
#pragma unroll 8
        for (int k = 0; k < a.cin; k += 2) {
            const int kk = k + h;
            const float b = (colok && kk < a.cin) ? wp[(size_t)kk * a.cout] : 0.f;
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(t0[k], b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(t1[k], b, acc1, 0, 0, 0);
        }
        if (!colok) continue;
        const float bv = a.bias ? a.bias[col] : 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = r0 + (j & 3) + 8 * (j >> 2) + 4 * h;
            if (row < a.n_nodes) {
                float v = acc0[j] + bv;
                if (a.relu) v = fmaxf(v, 0.f);
                a.out[(size_t)row * a.cout + col] = v;
            }
            if (row + 32 < a.n_nodes) {
                float v = acc1[j] + bv;
                if (a.relu) v = fmaxf(v, 0.f);
                a.out[(size_t)(row + 32) * a.cout + col] = v;
            }
        }
    }
}

GpdeLdsOnce gcn_lds_once;

template <bool HASW>
int gcn_launch(const GcnArgs& a, hipStream_t st) {
    const int np = (a.cin + 63) / 64;
    const dim3 grid((unsigned)((a.n_nodes + GCN_TM - 1) / GCN_TM)), block(256);
    const size_t lds = HASW ? (size_t)GCN_TM * a.kstride * sizeof(float) : 0;
    switch (np) {
        case 1: hipLaunchKernelGGL((gpde_gcn_fwd_kernel<1, HASW>), grid, block, lds, st, a); break;
        case 2: hipLaunchKernelGGL((gpde_gcn_fwd_kernel<2, HASW>), grid, block, lds, st, a); break;
        case 3: hipLaunchKernelGGL((gpde_gcn_fwd_kernel<3, HASW>), grid, block, lds, st, a); break;
        default: hipLaunchKernelGGL((gpde_gcn_fwd_kernel<4, HASW>), grid, block, lds, st, a); break;
    }
    GP_LAUNCH_CHECK("gpde_gcn_fwd_kernel");
    return GPDE_OK;
}

int gcn_check_widths(const char* who, int cin, int cout) {
    if (cin < 1 || cout < 1 || cin > GCN_MAXW || cout > GCN_MAXW) {
        gpde_set_error("%s: widths %d -> %d: built for 1 <= in_channels, out_channels <= %d (GPDE_WECONV_ANY_MAX_WIDTH)", who, cin, cout,
                       GCN_MAXW);
        return GPDE_EINVAL;
    }
    return GPDE_OK;
}

static inline size_t gcn_al(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

extern "C" size_t gpde_gcn_norm_workspace_bytes(int64_t n_nodes, int64_t n_edges) {
    if (n_nodes < 0 || n_edges < 0) return 0;
    return gcn_al((size_t)(n_nodes > 0 ? n_nodes : 1) * 8) + gcn_al((size_t)(n_nodes > 0 ? n_nodes : 1) * 4) + 256;   // dinv (double), selfw
}

extern "C" int gpde_gcn_norm(const int32_t* rowptr, const int32_t* src, const int32_t* perm, const float* edge_weight, int64_t n_nodes,
                             int64_t n_edges, uint32_t flags, float* coef, float* self_coef, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* who = "gpde_gcn_norm";
    if (n_nodes < 0 || n_edges < 0 || n_nodes >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31)) {
        gpde_set_error("%s: n_nodes %lld / n_edges %lld outside an int32 CSR", who, (long long)n_nodes, (long long)n_edges);
        return GPDE_EINVAL;
    }
    if (flags & ~(uint32_t)(GPDE_GCN_ADD_SELF_LOOPS | GPDE_GCN_IMPROVED | GPDE_GCN_NORMALIZE)) {
        gpde_set_error("%s: unknown flags %#x", who, flags);
        return GPDE_EINVAL;
    }
    if (n_nodes == 0) {
        if (n_edges > 0) {
            gpde_set_error("%s: %lld edges without nodes", who, (long long)n_edges);
            return GPDE_EINVAL;
        }
        return GPDE_OK;
    }
    if (!rowptr || !self_coef || (n_edges > 0 && (!src || !coef)) || (n_edges > 0 && edge_weight && !perm)) {
        gpde_set_error("%s: null rowptr / self_coef, null src / coef with edges, or edge_weight without perm", who);
        return GPDE_EINVAL;
    }
    if (!ws || ws_bytes < gpde_gcn_norm_workspace_bytes(n_nodes, n_edges)) {
        gpde_set_error("%s: workspace of %zu bytes, gpde_gcn_norm_workspace_bytes() asks for %zu", who, ws ? ws_bytes : (size_t)0,
                       gpde_gcn_norm_workspace_bytes(n_nodes, n_edges));
        return ws ? GPDE_EWORKSPACE : GPDE_EINVAL;
    }
    const int normalize = (flags & GPDE_GCN_NORMALIZE) ? 1 : 0;
    const int self_loops = (normalize && (flags & GPDE_GCN_ADD_SELF_LOOPS)) ? 1 : 0;
    const float fill = (flags & GPDE_GCN_IMPROVED) ? 2.f : 1.f;
    char* w = (char*)(((uintptr_t)ws + 255) / 256 * 256);
    double* dinv = (double*)w;
    float* selfw = (float*)(w + gcn_al((size_t)n_nodes * 8));
    const int n = (int)n_nodes;
    if (normalize) {
        hipLaunchKernelGGL(k_gcn_degree, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rowptr, src, perm, edge_weight, n, self_loops,
                           fill, dinv, selfw);
        GP_LAUNCH_CHECK("k_gcn_degree");
    }
    hipLaunchKernelGGL(k_gcn_coef, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, rowptr, src, perm, edge_weight, n, self_loops, normalize,
                       dinv, selfw, coef, self_coef);
    GP_LAUNCH_CHECK("k_gcn_coef");
    return GPDE_OK;
}

extern "C" int gpde_gcn_plan(int in_channels, int out_channels, int32_t* out) {
    if (!out) {
        gpde_set_error("gpde_gcn_plan: null out");
        return GPDE_EINVAL;
    }
    int rc = gcn_check_widths("gpde_gcn_plan", in_channels, out_channels);
    if (rc != GPDE_OK) return rc;
    const int ncb = (out_channels + 31) / 32;
    out[0] = GCN_TM;                              // destination rows per workgroup
    out[1] = gcn_kstride(in_channels);            // LDS row stride of the aggregated tile (floats)
    out[2] = (in_channels + 63) / 64;             // channel passes per lane in the aggregation
    out[3] = ncb;                                 // 32-column blocks of the product
    out[4] = (ncb + 3) / 4;                       // column blocks per wave
    out[5] = in_channels & 1;                     // K tail (the MFMA steps over k in pairs)
    out[6] = out_channels % 32 ? 1 : 0;           // column tail
    out[7] = GCN_TM * gcn_kstride(in_channels) * 4;   // LDS bytes
    return GPDE_OK;
}

extern "C" int gpde_gcn_fwd(const float* x, int64_t n_nodes, int64_t n_edges, const int32_t* rowptr, const int32_t* src, const float* coef,
                            const float* self_coef, const float* W, const float* bias, int in_channels, int out_channels, uint32_t flags,
                            float* out, float* agg_out, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* who = "gpde_gcn_fwd";
    if (n_nodes < 0 || n_edges < 0 || n_nodes >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31)) {
        gpde_set_error("%s: n_nodes %lld / n_edges %lld outside an int32 CSR", who, (long long)n_nodes, (long long)n_edges);
        return GPDE_EINVAL;
    }
    int rc = gcn_check_widths(who, in_channels, out_channels);
    if (rc != GPDE_OK) return rc;
    if (flags & ~(uint32_t)GPDE_GCN_RELU) {
        gpde_set_error("%s: unknown flags %#x", who, flags);
        return GPDE_EINVAL;
    }
    if (!W && in_channels != out_channels) {
        gpde_set_error("%s: W == NULL is the pure aggregation: out_channels must equal in_channels (%d -> %d)", who, in_channels, out_channels);
        return GPDE_EINVAL;
    }
    if (n_nodes == 0) {
        if (n_edges > 0) {
            gpde_set_error("%s: %lld edges without nodes", who, (long long)n_edges);
            return GPDE_EINVAL;
        }
        return GPDE_OK;
    }
    if (!x || !out || !rowptr || (n_edges > 0 && (!src || !coef))) {
        gpde_set_error("%s: null x / out / rowptr, or null src / coef with edges", who);
        return GPDE_EINVAL;
    }
    const size_t xb = (size_t)n_nodes * in_channels * 4;
    if (gp_overlap(out, (size_t)n_nodes * out_channels * 4, x, xb) || gp_overlap(agg_out, xb, x, xb) ||
        gp_overlap(agg_out, xb, out, (size_t)n_nodes * out_channels * 4)) {
        gpde_set_error("%s: out / agg_out overlap x or each other (other workgroups still gather those rows)", who);
        return GPDE_EINVAL;
    }
    GcnArgs a{x, rowptr, src, coef, self_coef, W, bias, out, agg_out, (int)n_nodes, in_channels, out_channels,
              (flags & GPDE_GCN_RELU) ? 1 : 0, gcn_kstride(in_channels)};
    if (!W) return gcn_launch<false>(a, st);
    rc = gcn_lds_once.ensure(gpde_gcn_fwd_kernel<1, true>, gpde_gcn_fwd_kernel<2, true>, gpde_gcn_fwd_kernel<3, true>,
                             gpde_gcn_fwd_kernel<4, true>);
    if (rc != GPDE_OK) return rc;
    return gcn_launch<true>(a, st);
}
