// The RE-ASSOCIATED operator at ANY width: 1 <= in_channels, out_channels <= 256, last hidden width 1 <= K <= 4096.
//
// gpde_weconv_any.hip runs the reference's own order at widths other than 64 -> 64: `weight = nn(pseudo)` materialised as
// [E][in * out] (nn_conv.py:274), in * out * 4 bytes and 2 K in out FLOP per edge.  For a Linear / ReLU chain and 'add' / 'mean'
// the aggregation is linear in the last Linear, so - as the 64-wide kernels have done since round 1 - the sum over
// the in-edges is taken first.  With H = relu(L_{n-1}(...)) [E][K] (rows in CSR slot order), W_last [in * out][K], b_last [in * out]:
//     Z'_d = [Z_d | S_d]     Z_d[i][k] = sum_{e -> d} x[src e][i] H[e][k],   S_d[i] = sum_{e -> d} x[src e][i]        [in][KP]
//     P[(i, k)][o] = W_last[i out + o][k],   P[(i, K)][o] = b_last[i out + o]                                     [in KP][outP]
//     out_d = (Z'_d . P) (/ max(deg_d, 1) for 'mean') + x_d . root + bias
// KP = K + 1 rounded up to 4, outP = out rounded up to 4 (zero padding: the fp32 GEMM of gpde_gemm.hip loads 16 bytes at a time).
// Per-edge memory is K * 4 bytes; the last layer costs 2 E in K + 2 N in K out FLOP.
//     backward   g = grad_out (/ max(deg, 1));  dZ' = g . P^T;  dP += Z'^T . g (Z' of the node block RECOMPUTED, not kept);
//                dH[e][k] = sum_i x[src e][i] dZ_d[i][k];  dxe[e][i] = sum_k dZ_d[i][k] H[e][k], summed per source in ascending
//                slot order (gpde_csr_source_order); grad_root / grad_bias as in gpde_weconv_any.hip.
// Z' is in * KP * 4 bytes per node (1 MiB at 256 x 1024): both directions walk blocks of destination nodes sized to the workspace
// they are given, never smaller than one node.  fp32 throughout (fmaf, fp32 MFMA in the GEMMs): the f16 split needs scale bounds
// that do not exist at run-time widths.  No atomics; every sum in an order fixed by the shapes (and, for grad_w_last / grad_b_last
// alone, by the number of node blocks): two identical calls give identical bits.
//
// Kernels of this file:
//   gpde_reassoc_zagg_kernel      one workgroup per (node, 64 rows i, LK columns k): lanes along k read H rows coalesced, the x_j
//                                 rows of a pass of 32 in-edges are gathered into LDS once; in-edges in ascending slot order; the
//                                 products of a pass are summed on their own and the pass's partial added to the running sum (a
//                                 hub row of 8,192 in-edges is 256 additions deep, not 8,192: DESIGN.md §3)
//   gpde_reassoc_edge_bwd_kernel  one workgroup per (node, row segment): passes of 8 in-edges; dH with lanes along k (dZ_d rows read
//                                 coalesced, the 8 x_j rows in LDS), dxe with one wave per row i and an xor-shuffle tree over k
//   k_ra_permute / k_ra_unpermute the last Linear into P and dP back into torch's layouts: 32 x 32 tiles through LDS
//   k_ra_scale_g / k_ra_epilogue  g / deg of a node block;  split-K sum, mean, x . root + bias
// Two node sets (gpde_nnconv_*_hidden_bip): the aggregation and the per-edge backward gather x_src [n_src][in], the node blocks walk the
// n_dst destinations, the epilogue's root term and grad_root read x_dst [n_dst][in_dst]; the square entry points hand x for both.
#include "gpde_common.h"

namespace {

constexpr int RA_MAXW = GPDE_WECONV_ANY_MAX_WIDTH;
constexpr int RA_MAXK = GPDE_REASSOC_ANY_MAX_HIDDEN;
constexpr int RA_ROWS = 64;                      // rows i of Z' per workgroup of the aggregation
constexpr int RA_PE = 32;                        // in-edges per pass of the aggregation
constexpr int RB_PE = 8;                         // in-edges per pass of the per-edge backward
constexpr int RB_SEGS = 8;                       // workgroups sharing one destination row in the per-edge backward
constexpr int RA_MAX_SPLITS = 32;                // split-K partials of out = Z' . P
constexpr size_t RA_PREF_Z_BYTES = (size_t)512 << 20;   // Z' of the preferred node block

inline size_t ra_al(size_t b) { return (b + 255) / 256 * 256; }
inline int ra_pad4(int v) { return (v + 3) / 4 * 4; }

// Z'[d][i][k], d = node - node0: k < K the sum of x_j[i] H[e][k], k == K the sum of x_j[i], K < k < KP zero
template <int LK, int IT>
__global__ __launch_bounds__(256) void gpde_reassoc_zagg_kernel(const float* __restrict__ x, const float* __restrict__ H,
                                                                const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                                                                float* __restrict__ Z, int node0, int cin, int K, int KP) {
    static_assert(256 / LK * IT == RA_ROWS && IT % 4 == 0, "64 rows per workgroup");
    __shared__ __attribute__((aligned(16))) float xs[RA_PE * RA_ROWS];
    const int tid = threadIdx.x;
    const int kl = tid % LK, ig = tid / LK;
    const int d = blockIdx.x;
    const int k = blockIdx.y * LK + kl;
    const int i0 = blockIdx.z * RA_ROWS;
    const int r0 = rowptr[node0 + d], r1 = rowptr[node0 + d + 1];
    const float hfix = k == K ? 1.f : 0.f;      // the S_d column and the padding
    float acc[IT];
#pragma unroll
    for (int r = 0; r < IT; ++r) acc[r] = 0.f;
    for (int eb = r0; eb < r1; eb += RA_PE) {
        const int ne = r1 - eb < RA_PE ? r1 - eb : RA_PE;
        const int ne4 = (ne + 3) & ~3;
        __syncthreads();                                         // the previous pass's rows have been read
        for (int t = tid; t < ne4 * RA_ROWS; t += 256) {
            const int ee = t / RA_ROWS, i = i0 + (t % RA_ROWS);
            xs[t] = (ee < ne && i < cin) ? x[(size_t)src[eb + ee] * cin + i] : 0.f;
        }
        __syncthreads();
        float part[IT];
#pragma unroll
        for (int r = 0; r < IT; ++r) part[r] = 0.f;
        for (int e4 = 0; e4 < ne4; e4 += 4) {                    // the H values of 4 edges in flight before the first FMA
            float h[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) h[u] = (k < K && e4 + u < ne) ? H[(size_t)(eb + e4 + u) * K + k] : hfix;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const f32x4* __restrict__ xr = (const f32x4*)&xs[(e4 + u) * RA_ROWS + ig * IT];
#pragma unroll
                for (int q = 0; q < IT / 4; ++q) {
                    const f32x4 v = xr[q];
#pragma unroll
                    for (int t = 0; t < 4; ++t) part[4 * q + t] = fmaf(v[t], h[u], part[4 * q + t]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < IT; ++r) acc[r] += part[r];
    }
    if (k >= KP) return;
#pragma unroll
    for (int r = 0; r < IT; ++r) {
        const int i = i0 + ig * IT + r;
        if (i < cin) Z[((size_t)d * cin + i) * KP + k] = acc[r];
    }
}

// dH[e][k] = sum_i x_j[i] dZ_d[i][k] (k < K);  dxe[e][i] = sum_{k < K} dZ_d[i][k] H[e][k] + dZ_d[i][K]   for the in-edges e of node d = node0 + blockIdx.x
__global__ __launch_bounds__(256) void gpde_reassoc_edge_bwd_kernel(const float* __restrict__ x, const float* __restrict__ H,
                                                                    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                                                                    const float* __restrict__ dZ, float* __restrict__ dH,
                                                                    float* __restrict__ dxe, int node0, int cin, int K, int KP) {
    __shared__ __attribute__((aligned(16))) float xsT[RA_MAXW * RB_PE];      // [i][8 edges of the pass]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = blockIdx.x;
    const int r0 = rowptr[node0 + d], r1 = rowptr[node0 + d + 1];
    const float* __restrict__ dz = dZ + (size_t)d * cin * KP;
    for (int eb = r0 + (int)blockIdx.y * RB_PE; eb < r1; eb += (int)gridDim.y * RB_PE) {
        const int ne = r1 - eb < RB_PE ? r1 - eb : RB_PE;
        __syncthreads();
        for (int t = tid; t < RB_PE * cin; t += 256) {
            const int ee = t / cin, i = t - ee * cin;
            xsT[i * RB_PE + ee] = ee < ne ? x[(size_t)src[eb + ee] * cin + i] : 0.f;
        }
        __syncthreads();
        for (int k = tid; k < K; k += 256) {
            float a[RB_PE];
#pragma unroll
            for (int u = 0; u < RB_PE; ++u) a[u] = 0.f;
#pragma unroll 4
            for (int i = 0; i < cin; ++i) {
                const float z = dz[(size_t)i * KP + k];
                const f32x4 x0 = *(const f32x4*)&xsT[i * RB_PE], x1 = *(const f32x4*)&xsT[i * RB_PE + 4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    a[t] = fmaf(x0[t], z, a[t]);
                    a[4 + t] = fmaf(x1[t], z, a[4 + t]);
                }
            }
#pragma unroll
            for (int u = 0; u < RB_PE; ++u)
                if (u < ne) dH[(size_t)(eb + u) * K + k] = a[u];
        }
        if (!dxe) continue;
        for (int i = wave; i < cin; i += 4) {
            float p[RB_PE];
#pragma unroll
            for (int u = 0; u < RB_PE; ++u) p[u] = 0.f;
            const float zs = dz[(size_t)i * KP + K];
            for (int k = lane; k < K; k += 64) {
                const float z = dz[(size_t)i * KP + k];
#pragma unroll
                for (int u = 0; u < RB_PE; ++u) p[u] = fmaf(z, u < ne ? H[(size_t)(eb + u) * K + k] : 0.f, p[u]);
            }
#pragma unroll
            for (int u = 0; u < RB_PE; ++u) {
                for (int s = 32; s >= 1; s >>= 1) p[u] += __shfl_xor(p[u], s);       // a fixed tree over the 64 lanes
                if (lane == 0 && u < ne) dxe[(size_t)(eb + u) * cin + i] = p[u] + zs;    // + dS_d[i]: the column of ones
            }
        }
    }
}

// P[(i KP + k)][o] = W[(i cout + o)][k] (k < K), b[i cout + o] (k == K), 0 (padding)
__global__ __launch_bounds__(256) void k_ra_permute(const float* __restrict__ W, const float* __restrict__ b, float* __restrict__ P,
                                                    int cout, int coutP, int K, int KP) {
    __shared__ float t[32][33];
    const int i = blockIdx.z, k0 = blockIdx.x * 32, o0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int o = o0 + r, k = k0 + tx;
        float v = 0.f;
        if (o < cout) {
            if (k < K) v = W[((size_t)i * cout + o) * K + k];
            else if (k == K && b) v = b[(size_t)i * cout + o];
        }
        t[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, o = o0 + tx;
        if (k < KP && o < coutP) P[((size_t)i * KP + k) * coutP + o] = t[tx][r];
    }
}

__global__ __launch_bounds__(256) void k_ra_unpermute(const float* __restrict__ dP, float* __restrict__ gW, float* __restrict__ gb,
                                                      int cout, int coutP, int K, int KP) {
    __shared__ float t[32][33];
    const int i = blockIdx.z, k0 = blockIdx.x * 32, o0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, o = o0 + tx;
        t[r][tx] = (k < KP && o < cout) ? dP[((size_t)i * KP + k) * coutP + o] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int o = o0 + r, k = k0 + tx;
        if (o >= cout) continue;
        if (k < K) {
            if (gW) gW[((size_t)i * cout + o) * K + k] = t[tx][r];
        } else if (k == K && gb) {
            gb[(size_t)i * cout + o] = t[tx][r];
        }
    }
}

// gs[d][o] = grad_out[node0 + d][o] (/ in-degree for 'mean'), zero in the padding columns
__global__ __launch_bounds__(256) void k_ra_scale_g(const float* __restrict__ g, const int32_t* __restrict__ rowptr, float* __restrict__ gs,
                                                    int node0, int nb, int cout, int coutP, int aggr) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)nb * coutP) return;
    const int d = (int)(idx / coutP), o = (int)(idx - (size_t)d * coutP);
    float v = 0.f;
    if (o < cout) {
        v = g[(size_t)(node0 + d) * cout + o];
        const int deg = rowptr[node0 + d + 1] - rowptr[node0 + d];
        if (aggr == GPDE_AGGR_MEAN && deg > 0) v = v / (float)deg;
    }
    gs[idx] = v;
}

// out[node0 + d][o] = (sum of the split-K partials, in order) (/ in-degree) + x . root + bias
// `x` is the DESTINATION node table and `cin` its width (in_dst; root is [in_dst][out]): a square call hands its one table
__global__ __launch_bounds__(256) void k_ra_epilogue(const float* __restrict__ part, int splits, size_t split_stride,
                                                     const float* __restrict__ x, const int32_t* __restrict__ rowptr,
                                                     const float* __restrict__ root, const float* __restrict__ bias, float* __restrict__ out,
                                                     int node0, int nb, int cin, int cout, int aggr) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)nb * cout) return;
    const int d = (int)(idx / cout), o = (int)(idx - (size_t)d * cout);
    const int i = node0 + d;
    float t = 0.f;
    for (int s = 0; s < splits; ++s) t += part[(size_t)s * split_stride + idx];
    const int deg = rowptr[i + 1] - rowptr[i];
    if (aggr == GPDE_AGGR_MEAN && deg > 0) t = t / (float)deg;   // scatter-mean: sum / clamp(count, 1)
    if (root) {                                                  // update(): + x_i . root   (nn_conv.py:279-280)
        const float* __restrict__ xr = x + (size_t)i * cin;
        float rs = 0.f;
        for (int c = 0; c < cin; ++c) rs = fmaf(xr[c], root[(size_t)c * cout + o], rs);
        t += rs;
    }
    if (bias) t += bias[o];
    out[(size_t)i * cout + o] = t;
}

using RaShape = GpdeRaShape;     // (gpde_common.h: gpde_chain_any.hip sizes its node blocks with it)

RaShape ra_shape(int cin, int cout, int K) {
    RaShape s{};
    s.cin = cin; s.cout = cout; s.K = K;
    s.coutP = ra_pad4(cout);
    s.KP = ra_pad4(K + 1);
    s.zrow = (size_t)cin * s.KP;
    s.p_bytes = ra_al(s.zrow * s.coutP * 4);
    // split-K of out = Z' . P by the K extent alone (in KP / 32 chunks of the GEMM): the same sums whatever the node block
    const int chunks = (int)((s.zrow + 31) / 32);
    s.splits = chunks / 64 < 1 ? 1 : (chunks / 64 > RA_MAX_SPLITS ? RA_MAX_SPLITS : chunks / 64);
    return s;
}

constexpr size_t RA_SLACK = 256 + 3 * 256;       // alignment of the workspace base and of the per-block buffers

size_t ra_fwd_fixed(const RaShape& s) { return s.p_bytes + RA_SLACK; }
size_t ra_fwd_per_node(const RaShape& s) { return s.zrow * 4 + (size_t)s.splits * s.cout * 4; }
// `cind`: the width of the destination table, whose droot partials [in_dst][out] the workspace holds (a square call: cin)
size_t ra_bwd_fixed(const RaShape& s, int64_t n_edges, int cind) {
    return 2 * s.p_bytes + ra_al((size_t)(n_edges > 0 ? n_edges : 1) * s.cin * 4) + gpde_any_node_grads_ws_bytes(cind, s.cout) + RA_SLACK;
}
size_t ra_bwd_per_node(const RaShape& s) { return 2 * s.zrow * 4 + (size_t)s.coutP * 4; }

int64_t ra_pref_block(const RaShape& s, int64_t n_nodes) {
    int64_t nb = (int64_t)(RA_PREF_Z_BYTES / (s.zrow * 4));
    if (nb < 1) nb = 1;
    if (nb > n_nodes) nb = n_nodes;
    return nb < 1 ? 1 : nb;
}

int ra_check(const char* who, int cin, int cout, int K, int aggr) {
    if (aggr != GPDE_AGGR_ADD && aggr != GPDE_AGGR_MEAN) {
        if (aggr == GPDE_AGGR_MAX) {
            gpde_set_error("%s: GPDE_AGGR_MAX: the maximum is not linear in the last Linear - built for GPDE_AGGR_ADD and GPDE_AGGR_MEAN", who);
            return GPDE_EUNSUPPORTED;
        }
        gpde_set_error("%s: unknown aggr %d", who, aggr);
        return GPDE_EINVAL;
    }
    if (cin < 1 || cout < 1 || cin > RA_MAXW || cout > RA_MAXW) {
        gpde_set_error("%s: in_channels %d -> out_channels %d: built for 1 <= in_channels, out_channels <= %d (GPDE_WECONV_ANY_MAX_WIDTH)",
                       who, cin, cout, RA_MAXW);
        return GPDE_EUNSUPPORTED;
    }
    if (K < 1 || K > RA_MAXK) {
        gpde_set_error("%s: last hidden width %d: built for 1 .. %d (GPDE_REASSOC_ANY_MAX_HIDDEN)", who, K, RA_MAXK);
        return GPDE_EUNSUPPORTED;
    }
    return GPDE_OK;
}

int ra_launch_permute(const RaShape& s, const float* w_last, const float* b_last, float* P, hipStream_t st) {
    hipLaunchKernelGGL(k_ra_permute, dim3((s.KP + 31) / 32, (s.coutP + 31) / 32, s.cin), dim3(256), 0, st, w_last, b_last, P, s.cout,
                       s.coutP, s.K, s.KP);
    GP_LAUNCH_CHECK("k_ra_permute");
    return GPDE_OK;
}

int ra_launch_zagg(const RaShape& s, const float* x, const float* H, const int32_t* rowptr, const int32_t* src, float* Z, int node0,
                   int nb, hipStream_t st) {
    const unsigned iz = (unsigned)((s.cin + RA_ROWS - 1) / RA_ROWS);
    if (s.KP > 32)
        hipLaunchKernelGGL((gpde_reassoc_zagg_kernel<64, 16>), dim3((unsigned)nb, (unsigned)((s.KP + 63) / 64), iz), dim3(256), 0, st, x, H,
                           rowptr, src, Z, node0, s.cin, s.K, s.KP);
    else
        hipLaunchKernelGGL((gpde_reassoc_zagg_kernel<16, 4>), dim3((unsigned)nb, (unsigned)((s.KP + 15) / 16), iz), dim3(256), 0, st, x, H,
                           rowptr, src, Z, node0, s.cin, s.K, s.KP);
    GP_LAUNCH_CHECK("gpde_reassoc_zagg_kernel");
    return GPDE_OK;
}

GpdeGemmArgs ra_gemm(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int a_kc, int b_kc) {
    GpdeGemmArgs g{};
    g.A = A; g.B = B; g.C = C;
    g.M = M; g.N = N; g.K = K;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.a_kcontig = a_kc; g.b_kcontig = b_kc;
    g.batches = 1; g.splits = 1;
    return g;
}

inline char* ra_base(void* ws) { return (char*)(((uintptr_t)ws + 255) / 256 * 256); }

}  // namespace

namespace {

// One block of destination nodes [na, na + nb) of the forward: Z' of the block, out = Z' . P, the epilogue
int ra_fwd_block(const RaShape& s, const float* x_src, const float* x_dst, const float* hidden, const int32_t* rowptr, const int32_t* src,
                 const float* P, const float* root, const float* bias, int aggr, int in_dst, float* out, float* Z, float* part, int na, int nb,
                 hipStream_t st) {
    const int cout = s.cout;
    int rc = ra_launch_zagg(s, x_src, hidden, rowptr, src, Z, na, nb, st);
    if (rc != GPDE_OK) return rc;
    GpdeGemmArgs g = ra_gemm(Z, P, part, nb, cout, (int)s.zrow, (int)s.zrow, s.coutP, cout, 1, 0);     // NN: Z' . P
    g.splits = s.splits;
    g.strideSplit = (size_t)nb * cout;
    rc = gpde_launch_gemm(g, st);
    if (rc != GPDE_OK) return rc;
    const size_t n = (size_t)nb * cout;
    hipLaunchKernelGGL(k_ra_epilogue, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, s.splits, (size_t)nb * cout, x_dst, rowptr,
                       root, bias, out, na, nb, in_dst, cout, aggr);
    GP_LAUNCH_CHECK("k_ra_epilogue");
    return GPDE_OK;
}

// One block of destination nodes of the backward: g of the block, dZ' = g . P^T, dP (+)= Z'^T . g (dP NULL: skipped), then dH and the
// per-edge dx rows of the block's in-edges
int ra_bwd_block(const RaShape& s, const float* x_src, const float* hidden, const int32_t* rowptr, const int32_t* src, const float* P,
                 int aggr, const float* grad_out, float* dZ, float* Z, float* gs, float* dP, int dp_accumulate, float* grad_hidden, float* dxe,
                 int na, int nb, hipStream_t st) {
    const int cin = s.cin, cout = s.cout;
    const size_t ng = (size_t)nb * s.coutP;
    hipLaunchKernelGGL(k_ra_scale_g, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, st, grad_out, rowptr, gs, na, nb, cout, s.coutP, aggr);
    GP_LAUNCH_CHECK("k_ra_scale_g");
    // NT: dZ' = g . P^T
    int rc = gpde_launch_gemm(ra_gemm(gs, P, dZ, nb, (int)s.zrow, s.coutP, s.coutP, s.coutP, (int)s.zrow, 1, 1), st);
    if (rc != GPDE_OK) return rc;
    if (dP) {                                                    // TN: dP (+)= Z'^T . g, Z' of the block recomputed
        rc = ra_launch_zagg(s, x_src, hidden, rowptr, src, Z, na, nb, st);
        if (rc != GPDE_OK) return rc;
        GpdeGemmArgs g = ra_gemm(Z, gs, dP, (int)s.zrow, cout, nb, (int)s.zrow, s.coutP, s.coutP, 0, 0);
        g.accumulate = dp_accumulate;
        rc = gpde_launch_gemm(g, st);
        if (rc != GPDE_OK) return rc;
    }
    hipLaunchKernelGGL(gpde_reassoc_edge_bwd_kernel, dim3((unsigned)nb, RB_SEGS), dim3(256), 0, st, x_src, hidden, rowptr, src, dZ, grad_hidden,
                       dxe, na, cin, s.K, s.KP);
    GP_LAUNCH_CHECK("gpde_reassoc_edge_bwd_kernel");
    return GPDE_OK;
}

// The node-side gradients of both backwards.  With edges: grad_x_src from the per-edge rows `dxe` (ordered), on one node set with the
// root term in the same launch.  Without (`dxe` NULL): the root term alone.  grad_root / grad_bias through `ngp`.
int ra_bwd_node_side(const float* x_dst, int64_t n_src, int64_t n_nodes, const float* dxe, const int32_t* src_rowptr, const int32_t* src_slots,
                     const float* root, const float* grad_out, float* grad_x_src, float* grad_x_dst, float* grad_root, float* grad_bias,
                     float* ngp, int cin, int cind, int cout, bool square, hipStream_t st) {
    int rc;
    if (square) {
        if (grad_x_src) {
            if (!dxe) GP_HIP_CHECK(gpde_zero_async(grad_x_src, (size_t)n_nodes * cin * 4, st));          // the root term alone, added to 0
            rc = gpde_launch_any_dx_finish(dxe, dxe ? src_rowptr : nullptr, dxe ? src_slots : nullptr, root, grad_out, grad_x_src, n_nodes, cin,
                                           cout, dxe ? 1 : 0, st);
            if (rc != GPDE_OK) return rc;
        }
    } else {
        if (grad_x_src && !dxe && n_src > 0) GP_HIP_CHECK(gpde_zero_async(grad_x_src, (size_t)n_src * cin * 4, st));
        if (grad_x_src && dxe) {                                 // the sources: the sum over their out-edges, no root term
            rc = gpde_launch_any_dx_finish(dxe, src_rowptr, src_slots, nullptr, nullptr, grad_x_src, n_src, cin, cout, 1, st);
            if (rc != GPDE_OK) return rc;
        }
        if (grad_x_dst) {                                        // the destinations: g . root^T
            if (!root) GP_HIP_CHECK(gpde_zero_async(grad_x_dst, (size_t)n_nodes * cind * 4, st));
            else {
                rc = gpde_launch_any_dx_finish(nullptr, nullptr, nullptr, root, grad_out, grad_x_dst, n_nodes, cind, cout, 2, st);
                if (rc != GPDE_OK) return rc;
            }
        }
    }
    if (grad_root || grad_bias) {
        rc = gpde_launch_any_node_grads(x_dst, grad_out, ngp, n_nodes, cind, cout, grad_root, grad_bias, st);
        if (rc != GPDE_OK) return rc;
    }
    return GPDE_OK;
}

// Both forwards after their argument checks.  x_src [n_src][cin] is gathered by `src`; x_dst [n_dst][cind] (nullable with root
// == NULL) enters the epilogue's root term only; the node blocks walk the n_dst destinations.  A square call hands x twice.
int ra_fwd_run(const char* who, const float* x_src, const float* x_dst, int64_t n_nodes, const float* hidden, int64_t n_edges, int k_hidden,
               const int32_t* rowptr, const int32_t* src, const float* w_last, const float* b_last, const float* root, const float* bias,
               int aggr, int in_channels, int in_dst, int out_channels, float* out, void* ws, size_t ws_bytes, hipStream_t st) {
    int rc;
    const RaShape s = ra_shape(in_channels, out_channels, k_hidden);
    const int cout = s.cout;
    if (n_edges == 0) {                                          // no edge: update() alone
        const size_t n = (size_t)n_nodes * cout;
        hipLaunchKernelGGL(k_ra_epilogue, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)nullptr, 0, (size_t)0, x_dst, rowptr,
                           root, bias, out, 0, (int)n_nodes, in_dst, cout, aggr);
        GP_LAUNCH_CHECK("k_ra_epilogue");
        return GPDE_OK;
    }
    if (ws_bytes < ra_fwd_fixed(s) + ra_fwd_per_node(s)) {
        gpde_set_error("%s: workspace of %zu bytes holds less than one node's Z' (%zu bytes needed; %zu preferred)", who, ws_bytes,
                       ra_fwd_fixed(s) + ra_fwd_per_node(s),
                       gpde_nnconv_fwd_hidden_any_workspace_bytes(n_nodes, n_edges, in_channels, out_channels, k_hidden));
        return GPDE_EINVAL;
    }
    int64_t blk = (int64_t)((ws_bytes - ra_fwd_fixed(s)) / ra_fwd_per_node(s));
    if (blk > n_nodes) blk = n_nodes;
    char* w = ra_base(ws);
    float* P = (float*)w;
    float* Z = (float*)(w + s.p_bytes);
    float* part = (float*)((char*)Z + ra_al((size_t)blk * s.zrow * 4));
    rc = ra_launch_permute(s, w_last, b_last, P, st);
    if (rc != GPDE_OK) return rc;
    for (int64_t na = 0; na < n_nodes; na += blk) {
        const int nb = (int)(n_nodes - na < blk ? n_nodes - na : blk);
        rc = ra_fwd_block(s, x_src, x_dst, hidden, rowptr, src, P, root, bias, aggr, in_dst, out, Z, part, (int)na, nb, st);
        if (rc != GPDE_OK) return rc;
    }
    return GPDE_OK;
}

// Both backwards after their argument checks; n_nodes = the destinations (> 0).  `square`: one node set - grad_x_src [n_src = n_nodes]
// receives the root term in the same k_any_dx_finish launch as the source sum, grad_x_dst is unused.  Otherwise grad_x_src [n_src][cin]
// is the source sum alone and grad_x_dst [n_nodes][cind] = g . root^T.
int ra_bwd_run(const char* who, const float* x_src, int64_t n_src, const float* x_dst, int64_t n_nodes, const float* hidden, int64_t n_edges,
               int k_hidden, const int32_t* rowptr, const int32_t* src, const float* w_last, const float* b_last, const float* root, int aggr,
               int in_channels, int in_dst, int out_channels, const float* grad_out, float* grad_x_src, float* grad_x_dst, float* grad_hidden,
               float* grad_w_last, float* grad_b_last, float* grad_root, float* grad_bias, const int32_t* src_rowptr, const int32_t* src_slots,
               void* ws, size_t ws_bytes, bool square, hipStream_t st) {
    int rc;
    const RaShape s = ra_shape(in_channels, out_channels, k_hidden);
    const int cin = s.cin, cout = s.cout, cind = in_dst;
    if (n_edges == 0) {                                          // no edge: the node-side terms alone; only grad_root / grad_bias use the workspace
        if (grad_root || grad_bias) {
            if (!ws || ws_bytes < gpde_any_node_grads_ws_bytes(cind, cout) + 256) {
                gpde_set_error("%s: grad_root / grad_bias need %zu bytes of workspace", who, gpde_any_node_grads_ws_bytes(cind, cout) + 256);
                return GPDE_EINVAL;
            }
        }
        return ra_bwd_node_side(x_dst, n_src, n_nodes, nullptr, nullptr, nullptr, root, grad_out, grad_x_src, grad_x_dst, grad_root, grad_bias,
                                (grad_root || grad_bias) ? (float*)ra_base(ws) : nullptr, cin, cind, cout, square, st);
    }
    if (ws_bytes < ra_bwd_fixed(s, n_edges, cind) + ra_bwd_per_node(s)) {
        gpde_set_error("%s: workspace of %zu bytes holds less than one node's Z' and dZ' (%zu bytes needed; %zu preferred)", who, ws_bytes,
                       ra_bwd_fixed(s, n_edges, cind) + ra_bwd_per_node(s),
                       gpde_nnconv_bwd_hidden_bip_workspace_bytes(n_nodes, n_edges, in_channels, cind, out_channels, k_hidden));
        return GPDE_EINVAL;
    }
    char* w = ra_base(ws);
    float* P = (float*)w;
    float* dP = (float*)(w + s.p_bytes);
    float* dxe = (float*)(w + 2 * s.p_bytes);
    float* ngp = (float*)((char*)dxe + ra_al((size_t)n_edges * cin * 4));
    char* blkbuf = (char*)ngp + gpde_any_node_grads_ws_bytes(cind, cout);
    {
        int64_t blk = (int64_t)((ws_bytes - ra_bwd_fixed(s, n_edges, cind)) / ra_bwd_per_node(s));
        if (blk > n_nodes) blk = n_nodes;
        float* dZ = (float*)blkbuf;
        float* Z = (float*)((char*)dZ + ra_al((size_t)blk * s.zrow * 4));
        float* gs = (float*)((char*)Z + ra_al((size_t)blk * s.zrow * 4));
        const bool want_dp = grad_w_last || grad_b_last;
        rc = ra_launch_permute(s, w_last, b_last, P, st);
        if (rc != GPDE_OK) return rc;
        for (int64_t na = 0; na < n_nodes; na += blk) {
            const int nb = (int)(n_nodes - na < blk ? n_nodes - na : blk);
            rc = ra_bwd_block(s, x_src, hidden, rowptr, src, P, aggr, grad_out, dZ, Z, gs, want_dp ? dP : (float*)nullptr, na > 0 ? 1 : 0,
                              grad_hidden, grad_x_src ? dxe : (float*)nullptr, (int)na, nb, st);
            if (rc != GPDE_OK) return rc;
        }
        if (want_dp) {
            hipLaunchKernelGGL(k_ra_unpermute, dim3((s.KP + 31) / 32, (s.coutP + 31) / 32, cin), dim3(256), 0, st, dP, grad_w_last,
                               grad_b_last, cout, s.coutP, s.K, s.KP);
            GP_LAUNCH_CHECK("k_ra_unpermute");
        }
    }
    return ra_bwd_node_side(x_dst, n_src, n_nodes, dxe, src_rowptr, src_slots, root, grad_out, grad_x_src, grad_x_dst, grad_root, grad_bias, ngp,
                            cin, cind, cout, square, st);
}

int ra_check_in_dst(const char* who, int in_dst) {
    if (in_dst < 1 || in_dst > RA_MAXW) {
        gpde_set_error("%s: in_dst %d: built for 1 <= in_dst <= %d (GPDE_WECONV_ANY_MAX_WIDTH)", who, in_dst, RA_MAXW);
        return GPDE_EUNSUPPORTED;
    }
    return GPDE_OK;
}

}  // namespace

extern "C" size_t gpde_nnconv_fwd_hidden_any_workspace_bytes(int64_t n_nodes, int64_t n_edges, int in_channels, int out_channels,
                                                             int k_hidden) {
    if (n_nodes < 0 || n_edges < 0 || in_channels < 1 || out_channels < 1 || in_channels > RA_MAXW || out_channels > RA_MAXW ||
        k_hidden < 1 || k_hidden > RA_MAXK)
        return 0;
    const RaShape s = ra_shape(in_channels, out_channels, k_hidden);
    return ra_fwd_fixed(s) + (size_t)ra_pref_block(s, n_nodes) * ra_fwd_per_node(s);
}

// the forward's workspace holds P and Z' of a block of DESTINATION nodes: neither depends on the source count or on in_dst
extern "C" size_t gpde_nnconv_fwd_hidden_bip_workspace_bytes(int64_t n_dst, int64_t n_edges, int in_src, int out_channels, int k_hidden) {
    return gpde_nnconv_fwd_hidden_any_workspace_bytes(n_dst, n_edges, in_src, out_channels, k_hidden);
}

extern "C" int gpde_nnconv_fwd_hidden_any(const float* x, int64_t n_nodes, const float* hidden, int64_t n_edges, int k_hidden,
                                          const int32_t* rowptr, const int32_t* src, const float* w_last, const float* b_last,
                                          const float* root, const float* bias, int aggr, int in_channels, int out_channels, float* out,
                                          void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* who = "gpde_nnconv_fwd_hidden_any";
    if (n_nodes < 0 || n_edges < 0 || !rowptr || (n_nodes > 0 && (!x || !out)) || (n_edges > 0 && (!hidden || !src || !w_last || !ws)) ||
        n_nodes >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31)) {
        gpde_set_error("%s: null/negative argument", who);
        return GPDE_EINVAL;
    }
    int rc = ra_check(who, in_channels, out_channels, k_hidden, aggr);
    if (rc != GPDE_OK) return rc;
    if (n_nodes == 0) return GPDE_OK;
    return ra_fwd_run(who, x, x, n_nodes, hidden, n_edges, k_hidden, rowptr, src, w_last, b_last, root, bias, aggr, in_channels, in_channels,
                      out_channels, out, ws, ws_bytes, st);
}

extern "C" int gpde_nnconv_fwd_hidden_bip(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst, const float* hidden,
                                          int64_t n_edges, int k_hidden, const int32_t* rowptr, const int32_t* src, const float* w_last,
                                          const float* b_last, const float* root, const float* bias, int aggr, int in_src, int in_dst,
                                          int out_channels, float* out, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* who = "gpde_nnconv_fwd_hidden_bip";
    if (n_src < 0 || n_dst < 0 || n_edges < 0 || !rowptr || (n_dst > 0 && !out) ||
        (n_edges > 0 && (!hidden || !src || !w_last || !ws || !x_src || n_src == 0 || n_dst == 0)) ||
        n_src >= ((int64_t)1 << 31) || n_dst >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31)) {
        gpde_set_error("%s: null/negative argument or edges without sources or destinations", who);
        return GPDE_EINVAL;
    }
    if (n_dst > 0 && root && !x_dst) {                           // (no destination: an empty table has no address)
        gpde_set_error("%s: root without x_dst: the root term is x_dst . root (pass root = NULL for a call without destination features)", who);
        return GPDE_EINVAL;
    }
    int rc = ra_check(who, in_src, out_channels, k_hidden, aggr);
    if (rc != GPDE_OK) return rc;
    rc = ra_check_in_dst(who, in_dst);
    if (rc != GPDE_OK) return rc;
    if (n_dst == 0) return GPDE_OK;
    return ra_fwd_run(who, x_src, x_dst, n_dst, hidden, n_edges, k_hidden, rowptr, src, w_last, b_last, root, bias, aggr, in_src, in_dst,
                      out_channels, out, ws, ws_bytes, st);
}

extern "C" size_t gpde_nnconv_bwd_hidden_any_workspace_bytes(int64_t n_nodes, int64_t n_edges, int in_channels, int out_channels,
                                                             int k_hidden) {
    if (n_nodes < 0 || n_edges < 0 || in_channels < 1 || out_channels < 1 || in_channels > RA_MAXW || out_channels > RA_MAXW ||
        k_hidden < 1 || k_hidden > RA_MAXK)
        return 0;
    const RaShape s = ra_shape(in_channels, out_channels, k_hidden);
    return ra_bwd_fixed(s, n_edges, in_channels) + (size_t)ra_pref_block(s, n_nodes) * ra_bwd_per_node(s);
}

extern "C" size_t gpde_nnconv_bwd_hidden_bip_workspace_bytes(int64_t n_dst, int64_t n_edges, int in_src, int in_dst, int out_channels,
                                                             int k_hidden) {
    if (n_dst < 0 || n_edges < 0 || in_src < 1 || in_dst < 1 || out_channels < 1 || in_src > RA_MAXW || in_dst > RA_MAXW ||
        out_channels > RA_MAXW || k_hidden < 1 || k_hidden > RA_MAXK)
        return 0;
    const RaShape s = ra_shape(in_src, out_channels, k_hidden);
    return ra_bwd_fixed(s, n_edges, in_dst) + (size_t)ra_pref_block(s, n_dst) * ra_bwd_per_node(s);
}

extern "C" int gpde_nnconv_bwd_hidden_any(const float* x, int64_t n_nodes, const float* hidden, int64_t n_edges, int k_hidden,
                                          const int32_t* rowptr, const int32_t* src, const float* w_last, const float* b_last,
                                          const float* root, int aggr, int in_channels, int out_channels, const float* grad_out,
                                          float* grad_x, float* grad_hidden, float* grad_w_last, float* grad_b_last, float* grad_root,
                                          float* grad_bias, const int32_t* src_rowptr, const int32_t* src_slots, void* ws, size_t ws_bytes,
                                          void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* who = "gpde_nnconv_bwd_hidden_any";
    if (n_nodes < 0 || n_edges < 0 || !rowptr || (n_nodes > 0 && (!x || !grad_out)) ||
        (n_edges > 0 && (!ws || !hidden || !src || !w_last || !grad_hidden || (grad_x && (!src_rowptr || !src_slots)))) ||
        n_nodes >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31)) {
        gpde_set_error("%s: null/negative argument (grad_hidden is required with edges, src_rowptr / src_slots with grad_x)", who);
        return GPDE_EINVAL;
    }
    int rc = ra_check(who, in_channels, out_channels, k_hidden, aggr);
    if (rc != GPDE_OK) return rc;
    const RaShape s = ra_shape(in_channels, out_channels, k_hidden);
    const int cin = s.cin, cout = s.cout;
    if (n_nodes == 0 || n_edges == 0) {                          // no edge: the last Linear received nothing
        if (grad_w_last) GP_HIP_CHECK(gpde_zero_async(grad_w_last, (size_t)cin * cout * s.K * 4, st));
        if (grad_b_last) GP_HIP_CHECK(gpde_zero_async(grad_b_last, (size_t)cin * cout * 4, st));
    }
    if (n_nodes == 0) {                                          // no node: sums over nothing, no workspace
        if (grad_root) GP_HIP_CHECK(gpde_zero_async(grad_root, (size_t)cin * cout * 4, st));
        if (grad_bias) GP_HIP_CHECK(gpde_zero_async(grad_bias, (size_t)cout * 4, st));
        return GPDE_OK;
    }
    return ra_bwd_run(who, x, n_nodes, x, n_nodes, hidden, n_edges, k_hidden, rowptr, src, w_last, b_last, root, aggr, in_channels,
                      in_channels, out_channels, grad_out, grad_x, nullptr, grad_hidden, grad_w_last, grad_b_last, grad_root, grad_bias,
                      src_rowptr, src_slots, ws, ws_bytes, true, st);
}

extern "C" int gpde_nnconv_bwd_hidden_bip(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst, const float* hidden,
                                          int64_t n_edges, int k_hidden, const int32_t* rowptr, const int32_t* src, const float* w_last,
                                          const float* b_last, const float* root, int aggr, int in_src, int in_dst, int out_channels,
                                          const float* grad_out, float* grad_x_src, float* grad_x_dst, float* grad_hidden,
                                          float* grad_w_last, float* grad_b_last, float* grad_root, float* grad_bias,
                                          const int32_t* src_rowptr, const int32_t* src_slots, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* who = "gpde_nnconv_bwd_hidden_bip";
    if (n_src < 0 || n_dst < 0 || n_edges < 0 || !rowptr || (n_dst > 0 && !grad_out) ||
        (n_edges > 0 && (!ws || !hidden || !src || !w_last || !grad_hidden || !x_src || n_src == 0 || n_dst == 0 ||
                         (grad_x_src && (!src_rowptr || !src_slots)))) ||
        n_src >= ((int64_t)1 << 31) || n_dst >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31)) {
        gpde_set_error("%s: null/negative argument (grad_hidden is required with edges, src_rowptr / src_slots over n_src with grad_x_src)", who);
        return GPDE_EINVAL;
    }
    if (n_dst > 0 && !x_dst && (root || grad_root || grad_x_dst)) {
        gpde_set_error("%s: root / grad_root / grad_x_dst without x_dst: the root term is x_dst . root", who);
        return GPDE_EINVAL;
    }
    int rc = ra_check(who, in_src, out_channels, k_hidden, aggr);
    if (rc != GPDE_OK) return rc;
    rc = ra_check_in_dst(who, in_dst);
    if (rc != GPDE_OK) return rc;
    const RaShape s = ra_shape(in_src, out_channels, k_hidden);
    if (n_dst == 0 || n_edges == 0) {                            // no edge: the last Linear received nothing
        if (grad_w_last) GP_HIP_CHECK(gpde_zero_async(grad_w_last, (size_t)s.cin * s.cout * s.K * 4, st));
        if (grad_b_last) GP_HIP_CHECK(gpde_zero_async(grad_b_last, (size_t)s.cin * s.cout * 4, st));
    }
    if (n_dst == 0) {                                            // no destination: sums over nothing, no workspace
        if (grad_x_src && n_src > 0) GP_HIP_CHECK(gpde_zero_async(grad_x_src, (size_t)n_src * in_src * 4, st));
        if (grad_root) GP_HIP_CHECK(gpde_zero_async(grad_root, (size_t)in_dst * s.cout * 4, st));
        if (grad_bias) GP_HIP_CHECK(gpde_zero_async(grad_bias, (size_t)s.cout * 4, st));
        return GPDE_OK;
    }
    return ra_bwd_run(who, x_src, n_src, x_dst, n_dst, hidden, n_edges, k_hidden, rowptr, src, w_last, b_last, root, aggr, in_src, in_dst,
                      out_channels, grad_out, grad_x_src, grad_x_dst, grad_hidden, grad_w_last, grad_b_last, grad_root, grad_bias, src_rowptr,
                      src_slots, ws, ws_bytes, false, st);
}

// ---- the node-block halves above for gpde_chain_any.hip (declared in gpde_common.h), which generates `hidden` block by block ----
GpdeRaShape gpde_ra_shape(int cin, int cout, int K) { return ra_shape(cin, cout, K); }
size_t gpde_ra_fwd_per_node(const GpdeRaShape& s) { return ra_fwd_per_node(s); }
size_t gpde_ra_bwd_per_node(const GpdeRaShape& s) { return ra_bwd_per_node(s); }
int64_t gpde_ra_pref_block(const GpdeRaShape& s, int64_t n_nodes) { return ra_pref_block(s, n_nodes); }
int gpde_ra_check(const char* who, int cin, int in_dst, int cout, int K, int aggr) {
    const int rc = ra_check(who, cin, cout, K, aggr);
    return rc != GPDE_OK ? rc : ra_check_in_dst(who, in_dst);
}
int gpde_ra_permute(const GpdeRaShape& s, const float* w_last, const float* b_last, float* P, hipStream_t st) {
    return ra_launch_permute(s, w_last, b_last, P, st);
}
int gpde_ra_unpermute(const GpdeRaShape& s, const float* dP, float* grad_w_last, float* grad_b_last, hipStream_t st) {
    hipLaunchKernelGGL(k_ra_unpermute, dim3((s.KP + 31) / 32, (s.coutP + 31) / 32, s.cin), dim3(256), 0, st, dP, grad_w_last, grad_b_last, s.cout,
                       s.coutP, s.K, s.KP);
    GP_LAUNCH_CHECK("k_ra_unpermute");
    return GPDE_OK;
}
int gpde_ra_fwd_block(const GpdeRaShape& s, const float* x_src, const float* x_dst, const float* hidden, const int32_t* rowptr,
                      const int32_t* src, const float* P, const float* root, const float* bias, int aggr, int in_dst, float* out, float* Z,
                      float* part, int na, int nb, hipStream_t st) {
    return ra_fwd_block(s, x_src, x_dst, hidden, rowptr, src, P, root, bias, aggr, in_dst, out, Z, part, na, nb, st);
}
int gpde_ra_bwd_block(const GpdeRaShape& s, const float* x_src, const float* hidden, const int32_t* rowptr, const int32_t* src, const float* P,
                      int aggr, const float* grad_out, float* dZ, float* Z, float* gs, float* dP, int dp_accumulate, float* grad_hidden,
                      float* dxe, int na, int nb, hipStream_t st) {
    return ra_bwd_block(s, x_src, hidden, rowptr, src, P, aggr, grad_out, dZ, Z, gs, dP, dp_accumulate, grad_hidden, dxe, na, nb, st);
}
int gpde_ra_bwd_node_side(const float* x_dst, int64_t n_src, int64_t n_nodes, const float* dxe, const int32_t* src_rowptr,
                          const int32_t* src_slots, const float* root, const float* grad_out, float* grad_x_src, float* grad_x_dst,
                          float* grad_root, float* grad_bias, float* ngp, int cin, int cind, int cout, bool square, hipStream_t st) {
    return ra_bwd_node_side(x_dst, n_src, n_nodes, dxe, src_rowptr, src_slots, root, grad_out, grad_x_src, grad_x_dst, grad_root, grad_bias, ngp,
                            cin, cind, cout, square, st);
}
