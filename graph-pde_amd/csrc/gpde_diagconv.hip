// The DIAGONAL-kernel operator: the reference's `NNConv` / `NNConv_Gaussian` (graph-neural-operator/nn_conv.py:8-96, 99-194), whose
// kernel network emits w values per edge that `diag_embed` turns into a diagonal w x w matrix - the message is x_j (.) k_e:
//     forward    out_i = aggr_{e: j -> i} x_src[j] (.) k_e  +  x_dst[i] . root + bias  (+ residual, ReLU)       nn_conv.py:83-92
//     backward   dk_e = x_j (.) gT_i,   grad_x_src[j] = sum_{e: j ->} k_e (.) gT_dst(e),   grad_x_dst = g . root^T,
//                grad_root = x_dst^T g,  grad_bias = colsum g                          (gT_i = g_i, / clamp(deg_i, 1) for 'mean')
// k is [E][w] fp32 in CSR slot order: 4 w bytes per edge where the full kernel of gpde_weconv_any.hip reads 4 w^2.  Streaming
// kernels under the HBM roof (4 w bytes of k_e and a gathered row of 4 w bytes for w FMAs), plain fp32, no matrix pipe, no
// floating-point atomics, every sum in an order fixed by the graph: two calls give the same bits.
//
// Work split: ONE WAVE (a 64-thread workgroup) per output row.  The lanes tile (edge slot, channel):
//     lc = lane % LC   column lanes.  w % 4 == 0: lane lc owns the four CONSECUTIVE channels 4 lc .. 4 lc + 3, LC = the power of two
//                      >= w / 4 - one 16-byte access per row when every buffer is 16-byte aligned (V = 4), else four dword accesses
//                      of the SAME channels (V = 1): the two read other instructions and add the same numbers in the same order.
//                      w % 4 != 0: lane lc owns channels lc, lc + LC, lc + 2 LC, lc + 3 LC, LC = the power of two >= min(w, 64).
//     es = lane / LC   ES = 64 / LC edge slots: at w = 64 four in-edges share the wave, at w = 8 thirty-two, at w = 256 one.
// A PASS is DG_U = 4 edges per slot: the indices, then the k_e rows and the gathered rows of 4 ES in-edges are issued before the
// first FMA (w = 64: 16 edges, 8 KiB in flight per wave).  A row is summed TWO-LEVEL: the products of DG_CH = 16
// passes (a chain of at most 64 edges per slot) into `part`, `part` into the slot's running sum, and at the end the ES slot sums
// in slot order - a hub row of 8,192 in-edges at w = 256 is 64 + 128 additions deep, not 8,192.
// The backward's source sum is THE SAME KERNEL on the transposed graph: rows = sources (gpde_csr_source_order's src_rowptr), the
// position p of a row names the CSR slot src_slots[p], the gathered table is gT and its row index dst[slot] - one owner per
// source, ascending slot order, no [E][w] intermediate.
// All offsets into k are size_t: E * w passes 2^31 at 8.4 M edges of w = 256.
#include "gpde_common.h"

namespace {

constexpr int DG_MAXW = GPDE_WECONV_ANY_MAX_WIDTH;
constexpr int DG_U = 4;              // edges per slot and pass: loads in flight before the first FMA
constexpr int DG_CH = 16;            // passes per chain (first level of the row sum)

static inline size_t dg_al(size_t b) { return (b + 255) / 256 * 256; }

// access modes of a lane's four values of one row
constexpr int DG_VEC4 = 0;           // channels 4 lc .. 4 lc + 3, one 16-byte access
constexpr int DG_CONSEC = 1;         // the same channels, four dword accesses (a buffer off a 16-byte boundary)
constexpr int DG_STRIDED = 2;        // channels lc + q LC (w % 4 != 0)

struct DiagPlan { int V, mode, LC, lcs, ES; };

DiagPlan diag_plan(int w, bool vec4) {
    DiagPlan p{};
    const bool consec = w % 4 == 0;
    p.mode = consec ? (vec4 ? DG_VEC4 : DG_CONSEC) : DG_STRIDED;
    p.V = p.mode == DG_VEC4 ? 4 : 1;
    const int ncl = consec ? w / 4 : w;
    p.LC = 1; p.lcs = 0;
    while (p.LC < ncl && p.LC < 64) { p.LC *= 2; ++p.lcs; }
    p.ES = 64 / p.LC;
    return p;
}

template <int MODE>
__device__ __forceinline__ void dg_load(float (&v)[4], const float* __restrict__ row, int lc, int LC, int w, bool on) {
    if constexpr (MODE == DG_VEC4) {
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if (on && 4 * lc < w) t = *(const f32x4*)(row + 4 * lc);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = t[q];
    } else if constexpr (MODE == DG_CONSEC) {
        const bool ok = on && 4 * lc < w;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = ok ? row[4 * lc + q] : 0.f;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int o = lc + q * LC;
            v[q] = (on && o < w) ? row[o] : 0.f;
        }
    }
}

template <int MODE>
__device__ __forceinline__ void dg_store(float* __restrict__ row, const float (&v)[4], int lc, int LC, int w) {
    if constexpr (MODE == DG_VEC4) {
        if (4 * lc < w) *(f32x4*)(row + 4 * lc) = f32x4{v[0], v[1], v[2], v[3]};
    } else if constexpr (MODE == DG_CONSEC) {
        if (4 * lc < w) {
#pragma unroll
            for (int q = 0; q < 4; ++q) row[4 * lc + q] = v[q];
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int o = lc + q * LC;
            if (o < w) row[o] = v[q];
        }
    }
}

struct DiagArgs {
    const float* x;            // the gathered table [n_gather][w]
    const float* k;            // [E][w], CSR slot order
    const int32_t* rowptr;     // [rows + 1] positions of each output row
    const int32_t* idx;        // [E] by CSR slot: the row of `x` an edge gathers
    const int32_t* slots;      // SLOTS: position -> CSR slot (the transposed graph); else position == slot
    const float* xd;           // [rows][cind] table of the root term
    const float* root;         // [cind][w] or NULL
    const float* bias; const float* residual; float* out;
    int n_gather, w, cind, aggr, relu, LC, lcs, ES;
};

template <int MODE, bool MAX, bool SLOTS>
__global__ __launch_bounds__(64) void gpde_diagconv_kernel(DiagArgs a) {
    __shared__ __attribute__((aligned(16))) float sm[64 * 8];
    const int lane = threadIdx.x;
    const int i = blockIdx.x;
    const int w = a.w, LC = a.LC, ES = a.ES;
    const int lc = lane & (LC - 1), es = lane >> a.lcs;
    const int r0 = a.rowptr[i], r1 = a.rowptr[i + 1];
    float acc[4], racc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = MAX ? -INFINITY : 0.f;

    const int pass = DG_U * ES;
    for (int c0 = r0; c0 < r1; c0 += DG_CH * pass) {             // a chain: the loops are wave-uniform, lanes past the row are masked
        const int c1 = min(r1, c0 + DG_CH * pass);
        float part[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) part[q] = MAX ? -INFINITY : 0.f;
        for (int pb = c0; pb < c1; pb += pass) {
            bool on[DG_U];
            int e[DG_U], j[DG_U];
#pragma unroll
            for (int u = 0; u < DG_U; ++u) {
                const int p = pb + u * ES + es;
                on[u] = p < c1;
                e[u] = on[u] ? (SLOTS ? a.slots[p] : p) : 0;
            }
#pragma unroll
            for (int u = 0; u < DG_U; ++u) {
                j[u] = on[u] ? a.idx[e[u]] : 0;
                if ((unsigned)j[u] >= (unsigned)a.n_gather) { j[u] = 0; on[u] = false; }      // (a CSR of the library has none: never read outside x)
            }
            float kv[DG_U][4], xv[DG_U][4];
#pragma unroll
            for (int u = 0; u < DG_U; ++u) {
                dg_load<MODE>(kv[u], a.k + (size_t)e[u] * w, lc, LC, w, on[u]);
                dg_load<MODE>(xv[u], a.x + (size_t)j[u] * w, lc, LC, w, on[u]);
            }
#pragma unroll
            for (int u = 0; u < DG_U; ++u)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if constexpr (MAX) part[q] = on[u] ? fmaxf(part[q], xv[u][q] * kv[u][q]) : part[q];
                    else part[q] = fmaf(xv[u][q], kv[u][q], part[q]);
                }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = MAX ? fmaxf(acc[q], part[q]) : acc[q] + part[q];
    }
    if (a.root) {                                                // update(): + x_dst[i] . root   (nn_conv.py:88-89)
        const float* __restrict__ xr = a.xd + (size_t)i * a.cind;
        for (int c = es; c < a.cind; c += ES) {
            float v[4];
            dg_load<MODE>(v, a.root + (size_t)c * w, lc, LC, w, true);
            const float xv = xr[c];
#pragma unroll
            for (int q = 0; q < 4; ++q) racc[q] = fmaf(xv, v[q], racc[q]);
        }
    }
    // the slots' sums, combined by the column's first lane in slot order: a fixed summation order
#pragma unroll
    for (int q = 0; q < 4; ++q) { sm[lane * 8 + q] = acc[q]; sm[lane * 8 + 4 + q] = racc[q]; }
    __syncthreads();
    if (es != 0) return;
    float t[4], rt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = MAX ? -INFINITY : 0.f;
    for (int s = 0; s < ES; ++s) {
        const float* p = sm + ((s << a.lcs) + lc) * 8;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            t[q] = MAX ? fmaxf(t[q], p[q]) : t[q] + p[q];
            rt[q] += p[4 + q];
        }
    }
    if (r1 == r0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = 0.f;                  // no in-edge: the aggregate is 0 (also for 'max')
    } else if (a.aggr == GPDE_AGGR_MEAN) {
        const float deg = (float)(r1 - r0);                      // scatter-mean: sum / clamp(count, 1)
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = t[q] / deg;
    }
    float bv[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) dg_load<MODE>(bv, a.bias, lc, LC, w, true);
    if (a.residual) dg_load<MODE>(rs, a.residual + (size_t)i * w, lc, LC, w, true);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        t[q] += rt[q];
        if (a.bias) t[q] += bv[q];
        if (a.residual) t[q] += rs[q];
        if (a.relu) t[q] = fmaxf(t[q], 0.f);
    }
    dg_store<MODE>(a.out + (size_t)i * w, t, lc, LC, w);
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// gT = g / clamp(deg, 1) ('mean'): one thread per element, formed once so that dk and the source sum read the same numbers
__global__ __launch_bounds__(256) void k_diag_gt(const float* __restrict__ g, const int32_t* __restrict__ rowptr, float* __restrict__ gt,
                                                 int64_t n_dst, int w) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n_dst * w) return;
    const size_t i = t / w;
    const int deg = rowptr[i + 1] - rowptr[i];
    gt[t] = deg > 1 ? g[t] / (float)deg : g[t];
}

struct DiagDkArgs {
    const float* x; const float* gt; const int32_t* rowptr; const int32_t* src; float* dk;
    int n_src, w, LC, lcs, ES;
};

// dk_e = x_j (.) gT_i: one wave per destination, the forward's lanes; the x_j rows of a pass in flight before the first store
template <int MODE>
__global__ __launch_bounds__(64) void gpde_diagconv_dk_kernel(DiagDkArgs a) {
    const int lane = threadIdx.x;
    const int i = blockIdx.x;
    const int w = a.w, LC = a.LC, ES = a.ES;
    const int lc = lane & (LC - 1), es = lane >> a.lcs;
    const int r0 = a.rowptr[i], r1 = a.rowptr[i + 1];
    if (r0 == r1) return;
    float gt[4];
    dg_load<MODE>(gt, a.gt + (size_t)i * w, lc, LC, w, true);
    for (int pb = r0; pb < r1; pb += DG_U * ES) {
        bool on[DG_U];
        int e[DG_U], j[DG_U];
#pragma unroll
        for (int u = 0; u < DG_U; ++u) {
            e[u] = pb + u * ES + es;
            on[u] = e[u] < r1;
            j[u] = on[u] ? a.src[e[u]] : 0;
            if ((unsigned)j[u] >= (unsigned)a.n_src) { j[u] = 0; on[u] = false; }
        }
        float xv[DG_U][4];
#pragma unroll
        for (int u = 0; u < DG_U; ++u) dg_load<MODE>(xv[u], a.x + (size_t)j[u] * w, lc, LC, w, on[u]);
#pragma unroll
        for (int u = 0; u < DG_U; ++u) {
            float o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = xv[u][q] * gt[q];
            if (e[u] < r1) dg_store<MODE>(a.dk + (size_t)e[u] * w, o, lc, LC, w);
        }
    }
}

bool dg_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int dg_check_width(const char* who, int w) {
    if (w < 1 || w > DG_MAXW) {
        gpde_set_error("%s: width %d: built for 1 <= width <= %d (GPDE_WECONV_ANY_MAX_WIDTH)", who, w, DG_MAXW);
        return GPDE_EUNSUPPORTED;
    }
    return GPDE_OK;
}

int dg_check_in_dst(const char* who, int in_dst) {
    if (in_dst < 1 || in_dst > DG_MAXW) {
        gpde_set_error("%s: in_dst %d: built for 1 <= in_dst <= %d (GPDE_WECONV_ANY_MAX_WIDTH)", who, in_dst, DG_MAXW);
        return GPDE_EUNSUPPORTED;
    }
    return GPDE_OK;
}

bool dg_known_aggr(int aggr) { return aggr == GPDE_AGGR_ADD || aggr == GPDE_AGGR_MEAN || aggr == GPDE_AGGR_MAX; }

template <bool MAX, bool SLOTS>
void dg_launch_mode(int mode, const DiagArgs& a, dim3 grid, hipStream_t st) {
    const dim3 block(64);
    switch (mode) {
        case DG_VEC4: hipLaunchKernelGGL((gpde_diagconv_kernel<DG_VEC4, MAX, SLOTS>), grid, block, 0, st, a); break;
        case DG_CONSEC: hipLaunchKernelGGL((gpde_diagconv_kernel<DG_CONSEC, MAX, SLOTS>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((gpde_diagconv_kernel<DG_STRIDED, MAX, SLOTS>), grid, block, 0, st, a); break;
    }
}

// the aggregation launch of the forward (slots == NULL) and of the backward's source sum (slots = src_slots)
int dg_launch(DiagArgs a, int64_t rows, hipStream_t st) {
    const bool vec4 = a.w % 4 == 0 && dg_aligned16(a.x) && dg_aligned16(a.k) && dg_aligned16(a.root) && dg_aligned16(a.bias) &&
                      dg_aligned16(a.residual) && dg_aligned16(a.out);
    const DiagPlan p = diag_plan(a.w, vec4);
    a.LC = p.LC; a.lcs = p.lcs; a.ES = p.ES;
    const dim3 grid((unsigned)rows);
    if (a.slots) dg_launch_mode<false, true>(p.mode, a, grid, st);
    else if (a.aggr == GPDE_AGGR_MAX) dg_launch_mode<true, false>(p.mode, a, grid, st);
    else dg_launch_mode<false, false>(p.mode, a, grid, st);
    GP_LAUNCH_CHECK("gpde_diagconv_kernel");
    return GPDE_OK;
}

}  // namespace

extern "C" int gpde_diagconv_plan(int width, int vec4, int aggr, int32_t* out) {
    if (!out || !dg_known_aggr(aggr)) {
        gpde_set_error("gpde_diagconv_plan: null out or unknown aggr");
        return GPDE_EINVAL;
    }
    int rc = dg_check_width("gpde_diagconv_plan", width);
    if (rc != GPDE_OK) return rc;
    const DiagPlan p = diag_plan(width, vec4 != 0);
    const int per_lane = p.mode == DG_STRIDED ? (width + p.LC - 1) / p.LC : 4;
    const int col_lanes = p.mode == DG_STRIDED ? (width < p.LC ? width : p.LC) : width / 4;
    out[0] = p.V;                       // floats per access: 4 or 1
    out[1] = p.LC;                      // column lanes (a power of two)
    out[2] = p.ES;                      // edge slots per wave
    out[3] = DG_U * p.ES;               // in-edges per pass
    out[4] = DG_CH * DG_U * p.ES;       // in-edges per chain (first level of the row sum)
    out[5] = p.LC * p.ES;               // lanes of the 64 that hold a slot
    out[6] = per_lane;                  // channels per column lane
    out[7] = p.mode == DG_STRIDED ? 0 : 1;      // 1: a lane's channels are consecutive (w % 4 == 0), 0: strided by LC
    out[8] = col_lanes * p.ES;          // lanes that own a channel
    out[9] = 64 * 8 * 4;                // LDS bytes (the slots' sums)
    return GPDE_OK;
}

extern "C" int gpde_diagconv_fwd(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst, const float* k, int64_t n_edges,
                                 const int32_t* rowptr, const int32_t* src, const float* root, const float* bias, const float* residual,
                                 int relu, int aggr, int width, int in_dst, float* out, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* who = "gpde_diagconv_fwd";
    if (n_src < 0 || n_dst < 0 || n_edges < 0 || n_src >= ((int64_t)1 << 31) || n_dst >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31)) {
        gpde_set_error("%s: n_src %lld / n_dst %lld / n_edges %lld outside an int32 CSR", who, (long long)n_src, (long long)n_dst,
                       (long long)n_edges);
        return GPDE_EINVAL;
    }
    if (!dg_known_aggr(aggr)) {
        gpde_set_error("%s: unknown aggr %d", who, aggr);
        return GPDE_EINVAL;
    }
    if (n_edges > 0 && (n_src == 0 || n_dst == 0)) {
        gpde_set_error("%s: %lld edges without sources or destinations", who, (long long)n_edges);
        return GPDE_EINVAL;
    }
    if (!rowptr || (n_dst > 0 && !out) || (n_edges > 0 && (!k || !src || !x_src))) {
        gpde_set_error("%s: null rowptr / out, or null k / src / x_src with edges", who);
        return GPDE_EINVAL;
    }
    if (n_dst > 0 && root && !x_dst) {
        gpde_set_error("%s: root without x_dst: the root term is x_dst . root (pass root = NULL for a call without destination features)", who);
        return GPDE_EINVAL;
    }
    if (residual && residual == out) {
        gpde_set_error("%s: residual aliases out", who);
        return GPDE_EINVAL;
    }
    int rc = dg_check_width(who, width);
    if (rc != GPDE_OK) return rc;
    rc = dg_check_in_dst(who, in_dst);
    if (rc != GPDE_OK) return rc;
    if (gp_overlap(out, (size_t)n_dst * width * 4, x_src, (size_t)n_src * width * 4)) {
        gpde_set_error("%s: out overlaps x_src (other waves still gather those rows)", who);
        return GPDE_EINVAL;
    }
    if (n_dst == 0) return GPDE_OK;
    DiagArgs a{x_src, k, rowptr, src, nullptr, x_dst, root, bias, residual, out, (int)n_src, width, in_dst, aggr, relu ? 1 : 0, 0, 0, 0};
    return dg_launch(a, n_dst, st);
}

extern "C" size_t gpde_diagconv_bwd_workspace_bytes(int64_t n_dst, int width, int in_dst) {
    if (n_dst < 0 || width < 1 || width > DG_MAXW || in_dst < 1 || in_dst > DG_MAXW) return 0;
    return dg_al((size_t)(n_dst > 0 ? n_dst : 1) * width * 4) +                     // gT [n_dst][w] ('mean')
           gpde_any_node_grads_ws_bytes(in_dst, width) + 1024;                      // grad_root / grad_bias strip partials
}

extern "C" int gpde_diagconv_bwd(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst, const float* k, int64_t n_edges,
                                 const int32_t* rowptr, const int32_t* src, const int32_t* dst, const int32_t* src_rowptr,
                                 const int32_t* src_slots, const float* root, int aggr, int width, int in_dst, const float* grad_out,
                                 float* grad_x_src, float* grad_x_dst, float* grad_k, float* grad_root, float* grad_bias, void* ws,
                                 size_t ws_bytes, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* who = "gpde_diagconv_bwd";
    if (n_src < 0 || n_dst < 0 || n_edges < 0 || n_src >= ((int64_t)1 << 31) || n_dst >= ((int64_t)1 << 31) || n_edges >= ((int64_t)1 << 31)) {
        gpde_set_error("%s: n_src %lld / n_dst %lld / n_edges %lld outside an int32 CSR", who, (long long)n_src, (long long)n_dst,
                       (long long)n_edges);
        return GPDE_EINVAL;
    }
    if (!dg_known_aggr(aggr)) {
        gpde_set_error("%s: unknown aggr %d", who, aggr);
        return GPDE_EINVAL;
    }
    if (n_edges > 0 && (n_src == 0 || n_dst == 0)) {
        gpde_set_error("%s: %lld edges without sources or destinations", who, (long long)n_edges);
        return GPDE_EINVAL;
    }
    if (!rowptr || !ws || (n_dst > 0 && !grad_out)) {
        gpde_set_error("%s: null rowptr / ws / grad_out", who);
        return GPDE_EINVAL;
    }
    if (n_edges > 0 && grad_k && (!src || !x_src)) {
        gpde_set_error("%s: grad_k needs src and x_src (dk_e = x_j (.) gT_i)", who);
        return GPDE_EINVAL;
    }
    if (n_edges > 0 && grad_x_src && (!k || !dst || !src_rowptr || !src_slots)) {
        gpde_set_error("%s: grad_x_src needs k, dst and src_rowptr / src_slots (gpde_csr_source_order): it is summed per source in ascending "
                       "slot order, never by atomics", who);
        return GPDE_EINVAL;
    }
    if (n_dst > 0 && !x_dst && (grad_root || grad_x_dst)) {
        gpde_set_error("%s: grad_root / grad_x_dst without x_dst: the root term is x_dst . root", who);
        return GPDE_EINVAL;
    }
    if ((grad_x_dst && grad_x_dst == grad_x_src) || (grad_k && (const float*)grad_k == k)) {
        gpde_set_error("%s: grad_x_dst aliases grad_x_src, or grad_k aliases k", who);
        return GPDE_EINVAL;
    }
    if (aggr == GPDE_AGGR_MAX) {
        gpde_set_error("%s: aggr %d: built for GPDE_AGGR_ADD and GPDE_AGGR_MEAN (the gradient of 'max' is composed by the caller)", who, aggr);
        return GPDE_EUNSUPPORTED;
    }
    int rc = dg_check_width(who, width);
    if (rc != GPDE_OK) return rc;
    rc = dg_check_in_dst(who, in_dst);
    if (rc != GPDE_OK) return rc;
    if (ws_bytes < gpde_diagconv_bwd_workspace_bytes(n_dst, width, in_dst)) {
        gpde_set_error("%s: workspace of %zu bytes, gpde_diagconv_bwd_workspace_bytes() asks for %zu", who, ws_bytes,
                       gpde_diagconv_bwd_workspace_bytes(n_dst, width, in_dst));
        return GPDE_EWORKSPACE;
    }
    const int w = width;
    // ONE node set: the caller hands one table twice and asks for no grad_x_dst - grad_x_src then holds both terms
    const bool fold = x_dst && x_dst == x_src && n_src == n_dst && in_dst == w && !grad_x_dst;
    if (n_dst == 0) {                                            // no destination: no edge either - every gradient is a sum over nothing
        if (grad_x_src && n_src > 0) GP_HIP_CHECK(gpde_zero_async(grad_x_src, (size_t)n_src * w * 4, st));
        if (grad_root) GP_HIP_CHECK(gpde_zero_async(grad_root, (size_t)in_dst * w * 4, st));
        if (grad_bias) GP_HIP_CHECK(gpde_zero_async(grad_bias, (size_t)w * 4, st));
        return GPDE_OK;
    }
    char* wsb = (char*)(((uintptr_t)ws + 255) / 256 * 256);
    float* gtbuf = (float*)wsb;
    float* part = (float*)(wsb + dg_al((size_t)n_dst * w * 4));
    const float* gt = grad_out;
    if (aggr == GPDE_AGGR_MEAN && n_edges > 0 && (grad_k || grad_x_src)) {
        const size_t n = (size_t)n_dst * w;
        hipLaunchKernelGGL(k_diag_gt, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, grad_out, rowptr, gtbuf, n_dst, w);
        GP_LAUNCH_CHECK("k_diag_gt");
        gt = gtbuf;
    }
    if (n_edges > 0 && grad_k) {
        const bool vec4 = w % 4 == 0 && dg_aligned16(x_src) && dg_aligned16(gt) && dg_aligned16(grad_k);
        const DiagPlan p = diag_plan(w, vec4);
        DiagDkArgs a{x_src, gt, rowptr, src, grad_k, (int)n_src, w, p.LC, p.lcs, p.ES};
        const dim3 grid((unsigned)n_dst), block(64);
        switch (p.mode) {
            case DG_VEC4: hipLaunchKernelGGL(gpde_diagconv_dk_kernel<DG_VEC4>, grid, block, 0, st, a); break;
            case DG_CONSEC: hipLaunchKernelGGL(gpde_diagconv_dk_kernel<DG_CONSEC>, grid, block, 0, st, a); break;
            default: hipLaunchKernelGGL(gpde_diagconv_dk_kernel<DG_STRIDED>, grid, block, 0, st, a); break;
        }
        GP_LAUNCH_CHECK("gpde_diagconv_dk_kernel");
    }
    if (grad_x_src && n_src > 0) {
        if (n_edges == 0) {
            GP_HIP_CHECK(gpde_zero_async(grad_x_src, (size_t)n_src * w * 4, st));
        } else {                                                 // the forward's loop on the transposed graph, one owner per source
            DiagArgs a{gt, k, src_rowptr, dst, src_slots, nullptr, nullptr, nullptr, nullptr, grad_x_src, (int)n_dst, w, w,
                       GPDE_AGGR_ADD, 0, 0, 0, 0};
            rc = dg_launch(a, n_src, st);
            if (rc != GPDE_OK) return rc;
        }
        if (fold && root) {                                      // + g . root^T on the same node set: grad_x_src[j][c] += sum_o root[c][o] g_j[o]
            rc = gpde_launch_any_dx_finish(nullptr, nullptr, nullptr, root, grad_out, grad_x_src, n_src, w, w, 0, st);
            if (rc != GPDE_OK) return rc;
        }
    }
    if (grad_x_dst) {
        if (!root) GP_HIP_CHECK(gpde_zero_async(grad_x_dst, (size_t)n_dst * in_dst * 4, st));
        else {
            rc = gpde_launch_any_dx_finish(nullptr, nullptr, nullptr, root, grad_out, grad_x_dst, n_dst, in_dst, w, 2, st);
            if (rc != GPDE_OK) return rc;
        }
    }
    if (grad_root || grad_bias) {
        if (!x_dst) {                                            // (grad_bias alone on a call without destination features)
            rc = gpde_launch_any_node_grads(grad_out, grad_out, part, n_dst, in_dst, w, nullptr, grad_bias, st);
        } else {
            rc = gpde_launch_any_node_grads(x_dst, grad_out, part, n_dst, in_dst, w, grad_root, grad_bias, st);
        }
        if (rc != GPDE_OK) return rc;
    }
    return GPDE_OK;
}
