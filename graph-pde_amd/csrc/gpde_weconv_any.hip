// The operator given the PER-EDGE WEIGHTS at ANY width: 1 <= in_channels, out_channels <= GPDE_WECONV_ANY_MAX_WIDTH (256).
//
// gpde_weconv.hip / gpde_weconv_bwd_kernel are written with lane = channel for 64 -> 64 (the width of every reference script).
// The reference's classes take any two widths (graph-neural-operator/nn_conv.py:234-241, message
// `nn(pseudo).view(-1, in_channels, out_channels)`, nn_conv.py:274); these kernels serve the others - and 64 -> 64 too, where the
// tests cross-check the two implementations.  W_e is [E][cin * cout] fp32, row-major [cin][cout] per edge, rows in CSR slot order:
//     forward    out_i = aggr_{e -> i} x_src(e) . W_e + x_i . root + bias  (+ residual, ReLU)          nn_conv.py:275, 277-282
//     backward   dW_e[c][o] = x_j[c] gT_i[o],  dx_j[c] = sum_{e: j ->} sum_o W_e[c][o] gT_i[o] + sum_o root[c][o] g_j[o],
//                droot = X^T g,  dbias = colsum g                                    (gT_i = g_i, / clamp(count_i, 1) for 'mean')
// Streaming kernels: cin * cout * 4 bytes per edge read once (forward), read once and written once (backward), ~2 FLOP per 4
// bytes - the roof is HBM.  Plain fp32 fmaf, no matrix pipe, no floating-point atomics (except grad_x when the caller gives no
// source order), every sum in an order fixed by the shapes alone: two runs give the same bits.
//
// Work split: ONE WAVE (a 64-thread workgroup) per destination node.  Inside the wave the lanes tile (edge slot, row, column):
//     lc = lane % LC   column lanes, consecutive along o: 16-byte accesses (V = 4) when cout % 4 == 0 and the buffers are
//                      16-byte aligned, else dword accesses (V = 1) with up to 4 column steps per lane; LC = the power of two
//                      >= min(cout / V, 64), so that the backward's dot products over o reduce with xor shuffles;
//     r            R = min(64 / LC, cin) row lanes: lane rows c = r, r + R, ... - the wave reads R * cout contiguous floats per
//                      step of an edge;
//     es           ES = 64 / LC / R edge slots: at 8 x 8 an edge is 256 B and 8 edges share the wave, at 128 x 128 (64 KiB)
//                      the whole wave streams one edge.
// The forward gathers the x_j rows of a batch of B * ES in-edges into LDS (<= 4 KiB), then issues the W_e rows of 4 edges before
// the first FMA (4 KiB in flight per wave, unrolled over two rows; at <= 64 VGPRs the SIMD holds 8 such waves).  The products of
// a batch are summed on their own and the batch's partial added to the node's running sum (a hub row of 8,192 in-edges of 256
// rows is then 2,048 additions deep, not 2 M: DESIGN.md §3 records the measured error before and after).
// Nodes of 2-3 in-edges cost one small wave each; a few hundred in-edges per node are one wave's sequential stream, and the
// machine is filled by the other nodes' waves (DESIGN.md §3 records the measured rates).
// All offsets into W_e are size_t: E * cin * cout passes 2^31 at 33 k edges of 256 x 256.
// Two node sets (gpde_nnconv_*_edgeweights_bip): x_src [n_src][cin] is what the edges gather, x_dst [n_dst][in_dst] enters the root term
// only (root [in_dst][out]), one wave per DESTINATION; grad_x_src [n_src][cin] is the source sum without a root term, grad_x_dst = g . root^T.
// The square entry points run the same launches with x_dst = x, in_dst = cin, n_src = n_dst: the same instructions on the same values.
#include "gpde_common.h"

namespace {

constexpr int ANY_MAXW = GPDE_WECONV_ANY_MAX_WIDTH;
constexpr int ANY_XS = 1024;            // floats of LDS per wave: the gathered x_j rows of one batch, then the partial sums

static inline size_t any_al(size_t b) { return (b + 255) / 256 * 256; }

struct AnyPlan { int V, LC, lcs, R, ES, B; };

// `max_mode`: every lane owns whole columns of its edges (R = 1) - the message of an edge must be complete before the maximum
AnyPlan any_plan(int cin, int cout, bool vec4, bool max_mode) {
    AnyPlan p{};
    p.V = vec4 ? 4 : 1;
    const int ncv = cout / p.V;
    p.LC = 1; p.lcs = 0;
    while (p.LC < ncv && p.LC < 64) { p.LC *= 2; ++p.lcs; }
    const int LR = 64 / p.LC;
    p.R = max_mode ? 1 : (LR < cin ? LR : cin);
    p.ES = LR / p.R;
    p.B = p.ES * cin <= 128 ? 8 : 4;       // B * ES * cin <= ANY_XS: ES * cin <= 64 when cin < LR, else ES = 1 and cin <= 256
    return p;
}

struct AnyFwdArgs {
    const float* x; const float* we; const int32_t* rowptr; const int32_t* src; const float* root; const float* bias;
    const float* residual; float* out;
    int cin, cout, aggr, relu, LC, lcs, R, ES, B;
    const float* xd; int cind;      // the DESTINATION node table [n_dst][cind] of the root term (a square call: xd = x, cind = cin)
};

// the lane's (up to) 4 values of one row: V = 4: columns 4 lc .. 4 lc + 3; V = 1: columns lc, lc + LC, lc + 2 LC, lc + 3 LC
template <int V>
__device__ __forceinline__ void row_load(float (&w)[4], const float* __restrict__ row, int lc, int LC, int cout, bool on) {
    if constexpr (V == 4) {
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if (on && 4 * lc < cout) t = *(const f32x4*)(row + 4 * lc);
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = t[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int o = lc + k * LC;
            w[k] = (on && o < cout) ? row[o] : 0.f;
        }
    }
}
template <int V>
__device__ __forceinline__ void row_store(float* __restrict__ row, const float (&w)[4], int lc, int LC, int cout) {
    if constexpr (V == 4) {
        if (4 * lc < cout) *(f32x4*)(row + 4 * lc) = f32x4{w[0], w[1], w[2], w[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int o = lc + k * LC;
            if (o < cout) row[o] = w[k];
        }
    }
}

template <int V, bool MAX>
__global__ __launch_bounds__(64) void gpde_weconv_any_kernel(AnyFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float sm[ANY_XS];
    const int lane = threadIdx.x;
    const int i = blockIdx.x;
    const int cin = a.cin, cout = a.cout, LC = a.LC, R = a.R, ES = a.ES;
    const int lc = lane & (LC - 1), lr = lane >> a.lcs;
    const int es = lr / R, r = lr - es * R;
    const bool lane_on = es < ES;
    const int r0 = a.rowptr[i], r1 = a.rowptr[i + 1];
    const size_t mat = (size_t)cin * cout;
    float acc[4], racc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = MAX ? -INFINITY : 0.f;

    if constexpr (MAX) {
        if (lane_on) {
            for (int e = r0 + es; e < r1; e += ES) {
                const float* __restrict__ xr = a.x + (size_t)a.src[e] * cin;
                const float* __restrict__ w = a.we + (size_t)e * mat;
                float m[4] = {0.f, 0.f, 0.f, 0.f};
                int c = 0;
                for (; c + 4 <= cin; c += 4) {
                    float v[4][4], xv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { row_load<V>(v[u], w + (size_t)(c + u) * cout, lc, LC, cout, true); xv[u] = xr[c + u]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int k = 0; k < 4; ++k) m[k] = fmaf(xv[u], v[u][k], m[k]);
                }
                for (; c < cin; ++c) {
                    float v[4];
                    row_load<V>(v, w + (size_t)c * cout, lc, LC, cout, true);
                    const float xv = xr[c];
#pragma unroll
                    for (int k = 0; k < 4; ++k) m[k] = fmaf(xv, v[k], m[k]);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = fmaxf(acc[k], m[k]);
            }
        }
    } else {
        const int B = a.B, EB = B * ES;
        for (int eb = r0; eb < r1; eb += EB) {
            const int ne = r1 - eb < EB ? r1 - eb : EB;
            __syncthreads();                                     // the previous batch's rows have been read
            for (int t = lane; t < ne * cin; t += 64) {
                const int ee = t / cin, c = t - ee * cin;
                sm[t] = a.x[(size_t)a.src[eb + ee] * cin + c];
            }
            __syncthreads();
            if (lane_on) {
                const float* __restrict__ wb = a.we + (size_t)eb * mat;
                // two-level sum: the pass's products into `part`, `part` into the running sum - a row of thousands of in-edges
                // adds one partial per pass instead of in_degree * in_channels / R products to one fp32 accumulator
                float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
                for (int c = r; c < cin; c += R) {
                    for (int b0 = 0; b0 < B; b0 += 4) {          // the row of 4 edges in flight before the first FMA
                        float v[4][4], xv[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int ee = (b0 + u) * ES + es;
                            const bool on = ee < ne;
                            row_load<V>(v[u], wb + (size_t)ee * mat + (size_t)c * cout, lc, LC, cout, on);
                            xv[u] = on ? sm[ee * cin + c] : 0.f;
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u)
#pragma unroll
                            for (int k = 0; k < 4; ++k) part[k] = fmaf(xv[u], v[u][k], part[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] += part[k];
            }
        }
    }
    if (a.root && es == 0) {                                     // update(): + x_i . root   (nn_conv.py:279-280)
        const int cind = a.cind;                                 // root is [in_dst][out], x_i a row of the destination table
        const float* __restrict__ xr = a.xd + (size_t)i * cind;
        for (int c = r; c < cind; c += R) {
            float v[4];
            row_load<V>(v, a.root + (size_t)c * cout, lc, LC, cout, true);
            const float xv = xr[c];
#pragma unroll
            for (int k = 0; k < 4; ++k) racc[k] = fmaf(xv, v[k], racc[k]);
        }
    }
    // the lanes' partials, combined by the column's first lane in (edge slot, row) order: a fixed summation order
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) { sm[lane * 8 + k] = acc[k]; sm[lane * 8 + 4 + k] = racc[k]; }
    __syncthreads();
    if (lr != 0) return;
    float t[4], rt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = MAX ? -INFINITY : 0.f;
    for (int s = 0; s < ES * R; ++s) {
        const float* p = sm + (size_t)((s << a.lcs) + lc) * 8;
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = MAX ? fmaxf(t[k], p[k]) : t[k] + p[k];
        if (s < R)
#pragma unroll
            for (int k = 0; k < 4; ++k) rt[k] += p[4 + k];
    }
    if (r1 == r0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = 0.f;                  // no in-edge: the aggregate is 0 (also for 'max')
    } else if (a.aggr == GPDE_AGGR_MEAN) {
        const float deg = (float)(r1 - r0);                      // scatter-mean: sum / clamp(count, 1)
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = t[k] / deg;
    }
    float bv[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) row_load<V>(bv, a.bias, lc, LC, cout, true);
    if (a.residual) row_load<V>(rs, a.residual + (size_t)i * cout, lc, LC, cout, true);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t[k] += rt[k];
        if (a.bias) t[k] += bv[k];
        if (a.residual) t[k] += rs[k];
        if (a.relu) t[k] = fmaxf(t[k], 0.f);
    }
    row_store<V>(a.out + (size_t)i * cout, t, lc, LC, cout);
}

// ---- backward --------------------------------------------------------------------------------------------------------------
struct AnyBwdArgs {
    const float* x; const float* we; const int32_t* rowptr; const int32_t* src; const float* g;
    float* dwe; float* dxe; float* dx;
    int cin, cout, aggr, LC, lcs, R, ES;
};

// One wave per destination node, lanes (edge slot, row, column) as in the forward.  Per row of an edge: W_e[c][.] read, dW_e[c][.]
// = x_j[c] gT_i written, and the dot product W_e[c][.] . gT_i reduced over the LC column lanes by xor shuffles (a fixed tree) into
// dxe[e][c] - the per-edge rows that k_any_dx_finish sums in source order (or, without a source order, an atomic on dx_j[c]).
// Four rows (loads and the x_j values) are in flight before the first store.
template <int V>
__global__ __launch_bounds__(64) void gpde_weconv_any_bwd_kernel(AnyBwdArgs a) {
    const int lane = threadIdx.x;
    const int i = blockIdx.x;
    const int cin = a.cin, cout = a.cout, LC = a.LC, R = a.R, ES = a.ES;
    const int lc = lane & (LC - 1), lr = lane >> a.lcs;
    const int es = lr / R, r = lr - es * R;
    const int r0 = a.rowptr[i], r1 = a.rowptr[i + 1];
    if (r0 == r1 || es >= ES) return;                            // (whole column groups leave together: the shuffles stay inside a group)
    const size_t mat = (size_t)cin * cout;
    float gt[4];
    row_load<V>(gt, a.g + (size_t)i * cout, lc, LC, cout, true);
    if (a.aggr == GPDE_AGGR_MEAN) {
        const float deg = (float)(r1 - r0);
#pragma unroll
        for (int k = 0; k < 4; ++k) gt[k] = gt[k] / deg;
    }
    for (int e = r0 + es; e < r1; e += ES) {
        const int j = a.src[e];
        const float* __restrict__ xr = a.x + (size_t)j * cin;
        const float* __restrict__ w = a.we + (size_t)e * mat;
        float* __restrict__ dw = a.dwe + (size_t)e * mat;
        for (int c = r; c < cin; c += 4 * R) {
            float v[4][4], xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int cu = c + u * R;
                const bool on = cu < cin;
                row_load<V>(v[u], w + (size_t)(on ? cu : c) * cout, lc, LC, cout, on);
                xv[u] = on ? xr[cu] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int cu = c + u * R;
                const bool on = cu < cin;
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = xv[u] * gt[k];
                if (on) row_store<V>(dw + (size_t)cu * cout, o, lc, LC, cout);
                float p = fmaf(v[u][3], gt[3], fmaf(v[u][2], gt[2], fmaf(v[u][1], gt[1], v[u][0] * gt[0])));
                for (int s = 1; s < LC; s <<= 1) p += __shfl_xor(p, s);
                if (on && lc == 0) {
                    if (a.dxe) a.dxe[(size_t)e * cin + cu] = p;
                    else atomicAdd(&a.dx[(size_t)j * cin + cu], p);
                }
            }
        }
    }
}

// grad_x[j][c] = (ordered == 1: sum over j's out-edges, ascending CSR slot, of dxe[slot][c]; 0: what the atomics left in grad_x;
//                 2: nothing) + sum_o root[c][o] g_j[o]                             one owner per element, sequential sums
// A square call has both terms on one node set.  A rectangular call runs it twice: over the n_src sources with root = NULL
// (grad_x_src has no root term) and over the n_dst destinations with ordered = 2 (grad_x_dst = g . root^T, cin = in_dst).
__global__ __launch_bounds__(256) void k_any_dx_finish(const float* __restrict__ dxe, const int32_t* __restrict__ srp,
                                                       const int32_t* __restrict__ ssl, const float* __restrict__ root,
                                                       const float* __restrict__ g, float* __restrict__ dx, int64_t n_nodes,
                                                       int cin, int cout, int ordered) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n_nodes * cin) return;
    const size_t j = idx / cin;
    const int c = (int)(idx - j * cin);
    float s = 0.f;
    if (ordered == 1) {
        const int p1 = srp[j + 1];
        for (int p = srp[j]; p < p1; ++p) s += dxe[(size_t)ssl[p] * cin + c];
    } else if (ordered == 0) {
        s = dx[idx];
    }
    if (root) {
        const float* __restrict__ rr = root + (size_t)c * cout;
        const float* __restrict__ gr = g + j * cout;
        float rs = 0.f;
        for (int o = 0; o < cout; ++o) rs = fmaf(rr[o], gr[o], rs);
        s += rs;
    }
    dx[idx] = s;
}

// droot = X^T g, dbias = colsum g (X the DESTINATION table, cin = in_dst, for a rectangular call): strip s of the nodes -> part[s][cin * cout + cout] (one thread per element, nodes in order),
// then the strips in order
__global__ __launch_bounds__(256) void k_any_node_grads(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ part,
                                                        int64_t n_nodes, int64_t strip, int cin, int cout, int do_root, int do_bias) {
    const int nrec = cin * cout + cout;
    const int el = blockIdx.x * 256 + threadIdx.x;
    if (el >= nrec) return;
    const int64_t n0 = (int64_t)blockIdx.y * strip;
    const int64_t n1 = n0 + strip < n_nodes ? n0 + strip : n_nodes;
    float s = 0.f;
    if (el < cin * cout) {
        if (!do_root) return;
        const int c = el / cout, o = el - c * cout;
        for (int64_t n = n0; n < n1; ++n) s = fmaf(x[(size_t)n * cin + c], g[(size_t)n * cout + o], s);
    } else {
        if (!do_bias) return;
        const int o = el - cin * cout;
        for (int64_t n = n0; n < n1; ++n) s += g[(size_t)n * cout + o];
    }
    part[(size_t)blockIdx.y * nrec + el] = s;
}
__global__ __launch_bounds__(256) void k_any_node_grads_reduce(const float* __restrict__ part, int nstrips, int cin, int cout,
                                                               float* __restrict__ droot, float* __restrict__ dbias) {
    const int nrec = cin * cout + cout;
    const int el = blockIdx.x * 256 + threadIdx.x;
    if (el >= nrec) return;
    float* out = el < cin * cout ? (droot ? droot + el : nullptr) : (dbias ? dbias + (el - cin * cout) : nullptr);
    if (!out) return;
    float s = 0.f;
    for (int k = 0; k < nstrips; ++k) s += part[(size_t)k * nrec + el];
    *out = s;
}

constexpr int ANY_MAX_STRIPS = 64;

bool any_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int any_check_widths(const char* who, int cin, int cout) {
    if (cin < 1 || cout < 1 || cin > ANY_MAXW || cout > ANY_MAXW) {
        gpde_set_error("%s: in_channels %d -> out_channels %d: built for 1 <= in_channels, out_channels <= %d (GPDE_WECONV_ANY_MAX_WIDTH)",
                       who, cin, cout, ANY_MAXW);
        return GPDE_EUNSUPPORTED;
    }
    return GPDE_OK;
}

}  // namespace

size_t gpde_any_node_grads_ws_bytes(int cin, int cout) {
    return any_al((size_t)ANY_MAX_STRIPS * ((size_t)cin * cout + cout) * 4);
}

int gpde_launch_any_dx_finish(const float* dxe, const int32_t* src_rowptr, const int32_t* src_slots, const float* root, const float* g,
                              float* dx, int64_t n_nodes, int cin, int cout, int ordered, hipStream_t st) {
    const size_t n = (size_t)n_nodes * cin;
    hipLaunchKernelGGL(k_any_dx_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dxe, src_rowptr, src_slots, root, g, dx,
                       n_nodes, cin, cout, ordered);
    GP_LAUNCH_CHECK("k_any_dx_finish");
    return GPDE_OK;
}

int gpde_launch_any_node_grads(const float* x, const float* g, float* part, int64_t n_nodes, int cin, int cout, float* droot,
                               float* dbias, hipStream_t st) {
    const int nrec = cin * cout + cout;
    int64_t nstrips = (n_nodes + 63) / 64;
    if (nstrips > ANY_MAX_STRIPS) nstrips = ANY_MAX_STRIPS;
    const int64_t strip = (n_nodes + nstrips - 1) / nstrips;
    nstrips = (n_nodes + strip - 1) / strip;
    const unsigned gx = (unsigned)((nrec + 255) / 256);
    hipLaunchKernelGGL(k_any_node_grads, dim3(gx, (unsigned)nstrips), dim3(256), 0, st, x, g, part, n_nodes, strip, cin, cout,
                       droot ? 1 : 0, dbias ? 1 : 0);
    hipLaunchKernelGGL(k_any_node_grads_reduce, dim3(gx), dim3(256), 0, st, part, (int)nstrips, cin, cout, droot, dbias);
    GP_LAUNCH_CHECK("k_any_node_grads");
    return GPDE_OK;
}

namespace {

// the launch of both forwards: the square call hands x for both tables
int any_fwd_launch(const float* x_src, const float* x_dst, int64_t n_dst, const float* edge_weights, const int32_t* rowptr,
                   const int32_t* src, const float* root, const float* bias, const float* residual, int relu, int aggr, int in_src,
                   int in_dst, int out_channels, float* out, hipStream_t st) {
    const bool vec4 = out_channels % 4 == 0 && any_aligned16(edge_weights) && any_aligned16(root) && any_aligned16(bias) &&
                      any_aligned16(residual) && any_aligned16(out);
    const bool is_max = aggr == GPDE_AGGR_MAX;
    const AnyPlan p = any_plan(in_src, out_channels, vec4, is_max);
    AnyFwdArgs a{x_src, edge_weights, rowptr, src, root, bias, residual, out,
                 in_src, out_channels, aggr, relu ? 1 : 0, p.LC, p.lcs, p.R, p.ES, p.B, x_dst, in_dst};
    const dim3 grid((unsigned)n_dst), block(64);
    if (vec4) {
        if (is_max) hipLaunchKernelGGL((gpde_weconv_any_kernel<4, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((gpde_weconv_any_kernel<4, false>), grid, block, 0, st, a);
    } else {
        if (is_max) hipLaunchKernelGGL((gpde_weconv_any_kernel<1, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((gpde_weconv_any_kernel<1, false>), grid, block, 0, st, a);
    }
    GP_LAUNCH_CHECK("gpde_weconv_any_kernel");
    return GPDE_OK;
}

// the launches of both backwards after their argument checks.  `square`: one node set - grad_x_src receives the root term in the
// same k_any_dx_finish launch as the source sum (the order of additions of the square call), grad_x_dst is unused.
int any_bwd_launch(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst, const float* edge_weights, int64_t n_edges,
                   const int32_t* rowptr, const int32_t* src, const int32_t* src_rowptr, const int32_t* src_slots, const float* root,
                   int aggr, int cin, int cind, int cout, const float* grad_out, float* grad_x_src, float* grad_x_dst,
                   float* grad_edge_weights, float* grad_root, float* grad_bias, void* ws, bool square, hipStream_t st) {
    int rc;
    char* w = (char*)(((uintptr_t)ws + 255) / 256 * 256);
    float* dxe = (float*)w;
    float* part = (float*)(w + any_al((size_t)(n_edges > 0 ? n_edges : 1) * cin * 4));
    const bool ordered = src_rowptr && src_slots;
    if (n_edges > 0) {
        const bool vec4 = cout % 4 == 0 && any_aligned16(edge_weights) && any_aligned16(grad_edge_weights) && any_aligned16(grad_out);
        const AnyPlan p = any_plan(cin, cout, vec4, false);
        if (grad_x_src && !ordered) GP_HIP_CHECK(gpde_zero_async(grad_x_src, (size_t)n_src * cin * 4, st));
        AnyBwdArgs a{x_src, edge_weights, rowptr, src, grad_out, grad_edge_weights, ordered ? dxe : nullptr, grad_x_src, cin, cout, aggr, p.LC, p.lcs, p.R, p.ES};
        if (!ordered && !grad_x_src) a.dxe = dxe;                // grad_x not wanted: the per-edge rows go to the workspace and are dropped
        if (vec4) hipLaunchKernelGGL(gpde_weconv_any_bwd_kernel<4>, dim3((unsigned)n_dst), dim3(64), 0, st, a);
        else hipLaunchKernelGGL(gpde_weconv_any_bwd_kernel<1>, dim3((unsigned)n_dst), dim3(64), 0, st, a);
        GP_LAUNCH_CHECK("gpde_weconv_any_bwd_kernel");
    }
    if (square) {
        if (grad_x_src) {
            if (n_edges == 0) GP_HIP_CHECK(gpde_zero_async(grad_x_src, (size_t)n_src * cin * 4, st));      // no edge: the root term alone, added to 0
            rc = gpde_launch_any_dx_finish(dxe, src_rowptr, src_slots, root, grad_out, grad_x_src, n_src, cin, cout, (ordered && n_edges > 0) ? 1 : 0, st);
            if (rc != GPDE_OK) return rc;
        }
    } else {
        if (grad_x_src && n_src > 0) {                           // the sources: the sum over their out-edges, no root term
            if (n_edges == 0) GP_HIP_CHECK(gpde_zero_async(grad_x_src, (size_t)n_src * cin * 4, st));
            else if (ordered) {
                rc = gpde_launch_any_dx_finish(dxe, src_rowptr, src_slots, nullptr, nullptr, grad_x_src, n_src, cin, cout, 1, st);
                if (rc != GPDE_OK) return rc;
            }                                                    // (atomics: grad_x_src is complete)
        }
        if (grad_x_dst) {                                        // the destinations: g . root^T
            if (!root) GP_HIP_CHECK(gpde_zero_async(grad_x_dst, (size_t)n_dst * cind * 4, st));
            else {
                rc = gpde_launch_any_dx_finish(nullptr, nullptr, nullptr, root, grad_out, grad_x_dst, n_dst, cind, cout, 2, st);
                if (rc != GPDE_OK) return rc;
            }
        }
    }
    if (grad_root || grad_bias) {
        rc = gpde_launch_any_node_grads(x_dst, grad_out, part, n_dst, cind, cout, grad_root, grad_bias, st);
        if (rc != GPDE_OK) return rc;
    }
    return GPDE_OK;
}

}  // namespace

extern "C" int gpde_nnconv_fwd_edgeweights_any(const float* x, int64_t n_nodes, const float* edge_weights, int64_t n_edges,
                                               const int32_t* rowptr, const int32_t* src, const float* root, const float* bias,
                                               const float* residual, int relu, int aggr, int in_channels, int out_channels,
                                               float* out, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    if (n_nodes < 0 || n_edges < 0 || !rowptr || (n_nodes > 0 && (!x || !out)) || (n_edges > 0 && (!edge_weights || !src)) ||
        (aggr != GPDE_AGGR_ADD && aggr != GPDE_AGGR_MEAN && aggr != GPDE_AGGR_MAX) || (residual && residual == out) ||
        n_nodes >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31)) {
        gpde_set_error("gpde_nnconv_fwd_edgeweights_any: null/negative argument, unknown aggr or residual aliases out");
        return GPDE_EINVAL;
    }
    int rc = any_check_widths("gpde_nnconv_fwd_edgeweights_any", in_channels, out_channels);
    if (rc != GPDE_OK) return rc;
    if (n_nodes == 0) return GPDE_OK;
    return any_fwd_launch(x, x, n_nodes, edge_weights, rowptr, src, root, bias, residual, relu, aggr, in_channels, in_channels,
                          out_channels, out, st);
}

extern "C" int gpde_nnconv_fwd_edgeweights_bip(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst,
                                               const float* edge_weights, int64_t n_edges, const int32_t* rowptr, const int32_t* src,
                                               const float* root, const float* bias, const float* residual, int relu, int aggr,
                                               int in_src, int in_dst, int out_channels, float* out, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* who = "gpde_nnconv_fwd_edgeweights_bip";
    if (n_src < 0 || n_dst < 0 || n_edges < 0 || !rowptr || (n_dst > 0 && !out) || (n_edges > 0 && (!edge_weights || !src || !x_src)) ||
        (n_edges > 0 && (n_src == 0 || n_dst == 0)) ||
        (aggr != GPDE_AGGR_ADD && aggr != GPDE_AGGR_MEAN && aggr != GPDE_AGGR_MAX) || (residual && residual == out) ||
        n_src >= ((int64_t)1 << 31) || n_dst >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31)) {
        gpde_set_error("%s: null/negative argument, edges without sources or destinations, unknown aggr or residual aliases out", who);
        return GPDE_EINVAL;
    }
    if (n_dst > 0 && root && !x_dst) {                           // (no destination: an empty table has no address)
        gpde_set_error("%s: root without x_dst: the root term is x_dst . root (pass root = NULL for a call without destination features)", who);
        return GPDE_EINVAL;
    }
    int rc = any_check_widths(who, in_src, out_channels);
    if (rc != GPDE_OK) return rc;
    if (in_dst < 1 || in_dst > ANY_MAXW) {
        gpde_set_error("%s: in_dst %d: built for 1 <= in_dst <= %d (GPDE_WECONV_ANY_MAX_WIDTH)", who, in_dst, ANY_MAXW);
        return GPDE_EUNSUPPORTED;
    }
    if (n_dst == 0) return GPDE_OK;
    return any_fwd_launch(x_src, x_dst, n_dst, edge_weights, rowptr, src, root, bias, residual, relu, aggr, in_src, in_dst, out_channels,
                          out, st);
}

extern "C" size_t gpde_nnconv_bwd_edgeweights_any_workspace_bytes(int64_t n_nodes, int64_t n_edges, int in_channels, int out_channels) {
    if (n_nodes < 0 || n_edges < 0 || in_channels < 1 || out_channels < 1 || in_channels > ANY_MAXW || out_channels > ANY_MAXW) return 0;
    return any_al((size_t)(n_edges > 0 ? n_edges : 1) * in_channels * 4) +                                   // dxe [E][cin]
           gpde_any_node_grads_ws_bytes(in_channels, out_channels) + 1024;                                   // droot / dbias partials
}

extern "C" size_t gpde_nnconv_bwd_edgeweights_bip_workspace_bytes(int64_t n_src, int64_t n_dst, int64_t n_edges, int in_src, int in_dst,
                                                                  int out_channels) {
    if (n_src < 0 || n_dst < 0 || n_edges < 0 || in_src < 1 || in_dst < 1 || out_channels < 1 || in_src > ANY_MAXW || in_dst > ANY_MAXW ||
        out_channels > ANY_MAXW)
        return 0;
    return any_al((size_t)(n_edges > 0 ? n_edges : 1) * in_src * 4) +                                        // dxe [E][in_src]
           gpde_any_node_grads_ws_bytes(in_dst, out_channels) + 1024;                                        // droot [in_dst][out] / dbias partials
}

extern "C" int gpde_nnconv_edgeweights_any_plan(int in_channels, int out_channels, int vec4, int aggr, int32_t* out) {
    if (!out || (aggr != GPDE_AGGR_ADD && aggr != GPDE_AGGR_MEAN && aggr != GPDE_AGGR_MAX)) {
        gpde_set_error("gpde_nnconv_edgeweights_any_plan: null out or unknown aggr");
        return GPDE_EINVAL;
    }
    int rc = any_check_widths("gpde_nnconv_edgeweights_any_plan", in_channels, out_channels);
    if (rc != GPDE_OK) return rc;
    const AnyPlan p = any_plan(in_channels, out_channels, vec4 && out_channels % 4 == 0, aggr == GPDE_AGGR_MAX);
    out[0] = p.V; out[1] = p.LC; out[2] = p.R; out[3] = p.ES; out[4] = p.B; out[5] = p.LC * p.R * p.ES;
    return GPDE_OK;
}

extern "C" int gpde_nnconv_bwd_edgeweights_any(const float* x, int64_t n_nodes, const float* edge_weights, int64_t n_edges,
                                               const int32_t* rowptr, const int32_t* src, const int32_t* src_rowptr,
                                               const int32_t* src_slots, const float* root, int aggr, int in_channels,
                                               int out_channels, const float* grad_out, float* grad_x, float* grad_edge_weights,
                                               float* grad_root, float* grad_bias, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    if (n_nodes < 0 || n_edges < 0 || !rowptr || !ws || (n_nodes > 0 && (!x || !grad_out)) ||
        (n_edges > 0 && (!edge_weights || !src || !grad_edge_weights)) || n_nodes >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31)) {
        gpde_set_error("gpde_nnconv_bwd_edgeweights_any: null/negative argument");
        return GPDE_EINVAL;
    }
    if (aggr != GPDE_AGGR_ADD && aggr != GPDE_AGGR_MEAN) {
        gpde_set_error("gpde_nnconv_bwd_edgeweights_any: aggr %d: built for GPDE_AGGR_ADD and GPDE_AGGR_MEAN (the gradient of 'max' is composed by the caller)", aggr);
        return GPDE_EUNSUPPORTED;
    }
    int rc = any_check_widths("gpde_nnconv_bwd_edgeweights_any", in_channels, out_channels);
    if (rc != GPDE_OK) return rc;
    if (ws_bytes < gpde_nnconv_bwd_edgeweights_any_workspace_bytes(n_nodes, n_edges, in_channels, out_channels)) {
        gpde_set_error("gpde_nnconv_bwd_edgeweights_any: workspace too small");
        return GPDE_EWORKSPACE;
    }
    if (n_nodes == 0) {
        // no node: grad_root / grad_bias are sums over nothing
        if (grad_root) GP_HIP_CHECK(gpde_zero_async(grad_root, (size_t)in_channels * out_channels * 4, st));
        if (grad_bias) GP_HIP_CHECK(gpde_zero_async(grad_bias, (size_t)out_channels * 4, st));
        return GPDE_OK;
    }
    return any_bwd_launch(x, n_nodes, x, n_nodes, edge_weights, n_edges, rowptr, src, src_rowptr, src_slots, root, aggr, in_channels,
                          in_channels, out_channels, grad_out, grad_x, nullptr, grad_edge_weights, grad_root, grad_bias, ws, true, st);
}

extern "C" int gpde_nnconv_bwd_edgeweights_bip(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst,
                                               const float* edge_weights, int64_t n_edges, const int32_t* rowptr, const int32_t* src,
                                               const int32_t* src_rowptr, const int32_t* src_slots, const float* root, int aggr,
                                               int in_src, int in_dst, int out_channels, const float* grad_out, float* grad_x_src,
                                               float* grad_x_dst, float* grad_edge_weights, float* grad_root, float* grad_bias,
                                               void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* who = "gpde_nnconv_bwd_edgeweights_bip";
    if (n_src < 0 || n_dst < 0 || n_edges < 0 || !rowptr || !ws || (n_dst > 0 && !grad_out) ||
        (n_edges > 0 && (!edge_weights || !src || !grad_edge_weights || !x_src || n_src == 0 || n_dst == 0)) ||
        n_src >= ((int64_t)1 << 31) || n_dst >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31)) {
        gpde_set_error("%s: null/negative argument or edges without sources or destinations", who);
        return GPDE_EINVAL;
    }
    if (n_dst > 0 && !x_dst && (root || grad_root || grad_x_dst)) {
        gpde_set_error("%s: root / grad_root / grad_x_dst without x_dst: the root term is x_dst . root", who);
        return GPDE_EINVAL;
    }
    if (aggr != GPDE_AGGR_ADD && aggr != GPDE_AGGR_MEAN) {
        gpde_set_error("%s: aggr %d: built for GPDE_AGGR_ADD and GPDE_AGGR_MEAN (the gradient of 'max' is composed by the caller)", who, aggr);
        return GPDE_EUNSUPPORTED;
    }
    int rc = any_check_widths(who, in_src, out_channels);
    if (rc != GPDE_OK) return rc;
    if (in_dst < 1 || in_dst > ANY_MAXW) {
        gpde_set_error("%s: in_dst %d: built for 1 <= in_dst <= %d (GPDE_WECONV_ANY_MAX_WIDTH)", who, in_dst, ANY_MAXW);
        return GPDE_EUNSUPPORTED;
    }
    if (ws_bytes < gpde_nnconv_bwd_edgeweights_bip_workspace_bytes(n_src, n_dst, n_edges, in_src, in_dst, out_channels)) {
        gpde_set_error("%s: workspace too small", who);
        return GPDE_EWORKSPACE;
    }
    if (n_dst == 0) {
        // no destination: no edge either - every gradient is a sum over nothing
        if (grad_x_src && n_src > 0) GP_HIP_CHECK(gpde_zero_async(grad_x_src, (size_t)n_src * in_src * 4, st));
        if (grad_root) GP_HIP_CHECK(gpde_zero_async(grad_root, (size_t)in_dst * out_channels * 4, st));
        if (grad_bias) GP_HIP_CHECK(gpde_zero_async(grad_bias, (size_t)out_channels * 4, st));
        return GPDE_OK;
    }
    return any_bwd_launch(x_src, n_src, x_dst, n_dst, edge_weights, n_edges, rowptr, src, src_rowptr, src_slots, root, aggr, in_src,
                          in_dst, out_channels, grad_out, grad_x_src, grad_x_dst, grad_edge_weights, grad_root, grad_bias, ws, false, st);
}
