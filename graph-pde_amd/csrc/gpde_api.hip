// C-ABI entry points of libgpde.so: launch planning and orchestration of the NNConv forward.
// Boundary replaced: nn_conv.NNConv_old.forward -> propagate -> message -> aggregate -> update
// (/root/reference/graph-neural-operator/nn_conv.py:267-282) — see include/gpde.h.
#include "gpde_common.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static thread_local char g_err[512] = "";

void gpde_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {
__global__ void k_zero_words(unsigned* __restrict__ p, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = 0u;
}
__global__ void k_zero_vec4(uint4* __restrict__ p, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = uint4{0u, 0u, 0u, 0u};
}
__global__ void k_zero2d_words(unsigned* __restrict__ p, size_t pitch_words, size_t width_words, size_t rows) {
    const size_t n = width_words * rows, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[(i / width_words) * pitch_words + i % width_words] = 0u;
}
__global__ void k_copy_words(unsigned* __restrict__ d, const unsigned* __restrict__ s_, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) d[i] = s_[i];
}
unsigned fill_blocks(size_t items) {
    size_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}
}  // namespace

hipError_t gpde_zero_async(void* p, size_t bytes, hipStream_t st) {
    if (bytes == 0) return hipSuccess;
    if (bytes % 4 != 0 || ((uintptr_t)p & 3)) return hipErrorInvalidValue;
    if (bytes % 16 == 0 && ((uintptr_t)p & 15) == 0) hipLaunchKernelGGL(k_zero_vec4, dim3(fill_blocks(bytes / 16)), dim3(256), 0, st, (uint4*)p, bytes / 16);
    else hipLaunchKernelGGL(k_zero_words, dim3(fill_blocks(bytes / 4)), dim3(256), 0, st, (unsigned*)p, bytes / 4);
    return hipGetLastError();
}
hipError_t gpde_zero2d_async(void* p, size_t pitch_bytes, size_t width_bytes, size_t rows, hipStream_t st) {
    if (width_bytes == 0 || rows == 0) return hipSuccess;
    if (pitch_bytes % 4 != 0 || width_bytes % 4 != 0 || ((uintptr_t)p & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_zero2d_words, dim3(fill_blocks(width_bytes / 4 * rows)), dim3(256), 0, st, (unsigned*)p, pitch_bytes / 4, width_bytes / 4, rows);
    return hipGetLastError();
}
hipError_t gpde_copy_async(void* dst, const void* src, size_t bytes, hipStream_t st) {
    if (bytes == 0) return hipSuccess;
    if (bytes % 4 != 0 || ((uintptr_t)dst & 3) || ((uintptr_t)src & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_copy_words, dim3(fill_blocks(bytes / 4)), dim3(256), 0, st, (unsigned*)dst, (const unsigned*)src, bytes / 4);
    return hipGetLastError();
}

namespace {
GpdeSwitches load_switches() {
    auto on = [](const char* n) { return getenv(n) != nullptr; };
    auto num = [](const char* n) { const char* e = getenv(n); return e ? atoi(e) : 0; };
    GpdeSwitches s{};
    s.bwd_gemm_f32 = on("GPDE_BWD_GEMM_F32");
    s.bwd_dw2_f32 = on("GPDE_BWD_DW2_F32");
    s.bwd_h1_materialize = on("GPDE_BWD_H1_MATERIALIZE");
    s.nt_no_prefetch = on("GPDE_NT_NO_PREFETCH");
    s.tn_no_ks_xcd = on("GPDE_TN_NO_KS_XCD");
    s.edge_bwd = num("GPDE_EDGE_BWD");
    const int v = num("GPDE_DEBUG_SKEW_US");
    s.debug_skew_us = v > 0 ? (v < 100000 ? v : 100000) : 0;
    return s;
}
GpdeSwitches& switches_storage() {
    static GpdeSwitches s = load_switches();        // first native call of the process (thread-safe static initialisation)
    return s;
}
}  // namespace

const GpdeSwitches& gpde_switches() { return switches_storage(); }

extern "C" int gpde_reload_switches(void) {
    switches_storage() = load_switches();
    return GPDE_OK;
}

// An ablation build (-DGPDE_ABL_*: part of the arithmetic removed, WRONG results, timing only) or an instrumented build
// (-DGPDE_*_TIMING: clock64 probes) says so in its version word; graph-pde_amd/_lib.py refuses the former unless asked.
#if defined(GPDE_ABL_2MFMA) || defined(GPDE_ABL_NOSTAGE) || defined(GPDE_ABL_NOBARRIER) || defined(GPDE_ABL_NOGEMM2) || defined(GPDE_ABL_NOWAIT) || defined(GPDE_BWABL)
#define GPDE_BUILD_FLAGS_ GPDE_VERSION_ABLATION
#elif defined(GPDE_V6_TIMING) || defined(GPDE_NT_TIMING) || defined(GPDE_EB2_TIMING) || defined(GPDE_V3_TIMING)
#define GPDE_BUILD_FLAGS_ GPDE_VERSION_INSTRUMENTED
#else
#define GPDE_BUILD_FLAGS_ 0
#endif
extern "C" int gpde_version(void) { return GPDE_VERSION | GPDE_BUILD_FLAGS_; }
extern "C" const char* gpde_last_error(void) { return g_err; }

namespace {

// ---- optional HIP-event timing of the kernels of gpde_nnconv_fwd (bench.py roofline leg) -------
struct EvPair { hipEvent_t a, b; int kind; };   // kind: GPDE_PROF_* (include/gpde.h)
thread_local bool g_prof_on = false;
thread_local std::vector<EvPair> g_prof;

struct ProfScope {
    bool on; EvPair p; hipStream_t s;
    ProfScope(int kind, hipStream_t stream) : on(g_prof_on), s(stream) {
        if (!on) return;
        p.kind = kind;
        if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(p.a, s);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(p.b, s);
        g_prof.push_back(p);
    }
};

constexpr size_t kAlign = 256;
size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

int num_cus_impl() {
    // per device (a process may drive several GPUs), cached after the first query
    static std::atomic<int> cus[32];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 31) dev = 0;
    int v = cus[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;   // MI355X
        cus[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

struct Plan {
    GpdePackLayout L;
    int64_t nodes_per_chunk;
    int n_chunks;
    int n_groups;        // fused-kernel edge groups (workgroups per hidden slice)
    size_t off_part, off_z, off_ha, off_hb, off_xs, off_scal, off_blk, off_img;
    bool attr_image;     // the attribute operand image of the f16v6 kernel has its place at off_img
    int nblk_max;        // f16v6 work queue: block-bound slots (0: no queue)
    size_t h_floats;     // mode 2: floats per ping-pong activation buffer
};

int pick_splits(int64_t nn) {
    // gemm3 streams Z from HBM with one 16 KiB chunk in flight per workgroup: ~1000 resident workgroups
    // (4 per CU) keep ~16 MB in flight, enough for the HBM latency-bandwidth product
    const int64_t tiles = (nn + 63) / 64;
    int s = 1;
    while (s < 64 && tiles * s < 1024) s *= 2;
    return s;
}

// Whether a forward call with these flags runs the f16v6 kernel on the attribute operand image (defined below, next to
// choose_fused)
bool attr_image_eligible(const GpdePackLayout& L, uint32_t flags, int64_t n_edges, int kt);

// `flags`, `kt`, `attr_given`: what decides whether the call can use the attribute operand image (sizing and the plan
// queries without flags: the default precision's).  Sizing sets its bytes aside wherever the forward would choose the
// f16v6 kernel; a plan for a given workspace takes the image only if, with those bytes set aside, it still gets the
// nodes per chunk that sizing recommends - otherwise it is the plan without the image, exactly
int make_plan(int64_t N, int64_t E, int n_layers, const int32_t* dims, size_t ws_bytes, bool sizing,
              Plan* P, size_t* needed, bool hidden_given = false, uint32_t flags = GPDE_FWD_F16SPLIT, int kt = 0,
              bool attr_given = true) {
    int rc = gpde_pack_layout(n_layers, dims, &P->L);
    if (rc != GPDE_OK) return rc;
    const GpdePackLayout& L = P->L;
    const size_t zrow = (size_t)GP_W * L.K2P * sizeof(float);
    const size_t prow = (size_t)64 * GP_W * sizeof(float);   // worst case: 64 splits
    size_t fixed = 0;
    P->h_floats = 0;
    // f16-split aggregation (mode 1): x as split f16 words [N][64] + two scalars (gpde_prep.hip)
    // (sized for every kernel shape: gpde_nnconv_fwd_hidden uses it whatever the MLP looks like)
    const size_t xs_bytes = (L.mode == 1 || hidden_given || sizing) ? align_up((size_t)(N > 0 ? N : 1) * GP_W * 4) + kAlign : 0;
    if (L.mode == 2 && !hidden_given) {
        int kmax = 0;
        for (int l = 1; l <= n_layers - 1; ++l) kmax = kmax > L.frontKP[l] ? kmax : L.frontKP[l];
        P->h_floats = (size_t)(E > 0 ? E : 1) * kmax;
        fixed = 2 * align_up(P->h_floats * sizeof(float));
    }
    fixed += xs_bytes;
    // f16v6 work queue: block bounds [nblk_max + 1] + block count + one counter per column slice
    P->nblk_max = (L.mode == 1 && E < ((int64_t)1 << 31) - GP_QBLOCK) ? (int)(E / GP_QBLOCK + E / 8 / (GP_QBLOCK / 8)) + 10 : 0;
    const size_t blk_bytes = P->nblk_max ? align_up(((size_t)P->nblk_max + 2 + 64) * 4) : 0;
    fixed += blk_bytes;
    const size_t img_bytes = (attr_given && !hidden_given && attr_image_eligible(L, flags, E, kt)) ? gpde_attr_image_bytes(E) : 0;
    // recommended: all nodes if Z fits 4 GiB, else 4 GiB worth of nodes (at least one tile)
    int64_t npc_rec = (int64_t)(((size_t)4 << 30) / zrow);
    if (npc_rec < 64) npc_rec = 64;
    if (npc_rec > N) npc_rec = N;
    if (npc_rec < 1) npc_rec = 1;
    // nodes per chunk of a given workspace with `fx` bytes outside the node chunks
    auto nodes_for = [&](size_t fx, bool quiet, int64_t* out) {
        if (ws_bytes < fx + 2 * kAlign) {
            if (!quiet) gpde_set_error("gpde_nnconv_fwd: workspace %zu bytes cannot hold the %zu-byte hidden "
                                       "activation buffers", ws_bytes, fx);
            return GPDE_EWORKSPACE;
        }
        int64_t n_ = (int64_t)((ws_bytes - fx - 2 * kAlign) / (zrow + prow));
        // the whole graph in one chunk whenever it fits exactly (the estimate above gives up two
        // alignment units, which used to split a graph sized with the recommended workspace)
        if (N > 0 && align_up((size_t)N * prow) + align_up((size_t)N * zrow) + fx <= ws_bytes) n_ = N;
        if (n_ > N) n_ = N;
        const int64_t min_nodes = N < 64 ? N : 64;
        if (n_ < min_nodes || (N > 0 && n_ < 1)) {
            if (!quiet) gpde_set_error("gpde_nnconv_fwd: workspace %zu bytes holds %lld destination nodes, need >= %lld "
                                       "(%zu bytes per node)", ws_bytes, (long long)n_, (long long)min_nodes, zrow + prow);
            return GPDE_EWORKSPACE;
        }
        if (n_ < N && n_ > 64) n_ = n_ / 64 * 64;
        *out = n_;
        return GPDE_OK;
    };
    int64_t npc;
    P->attr_image = false;
    if (sizing) {
        npc = npc_rec;
        P->attr_image = img_bytes != 0;
    } else {
        int64_t npc_img = 0;
        if (img_bytes && nodes_for(fixed + img_bytes, true, &npc_img) == GPDE_OK && npc_img >= npc_rec) {
            npc = npc_img;
            P->attr_image = true;
        } else if ((rc = nodes_for(fixed, false, &npc)) != GPDE_OK) {
            return rc;
        }
    }
    if (npc < 1) npc = 1;
    P->nodes_per_chunk = npc;
    P->n_chunks = (int)((N + npc - 1) / npc);
    if (P->n_chunks < 1) P->n_chunks = 1;
    size_t off = 0;
    P->off_part = off; off += align_up((size_t)npc * prow);
    P->off_z = off;    off += align_up((size_t)npc * zrow);
    P->off_ha = off;   off += (L.mode == 2 && !hidden_given) ? align_up(P->h_floats * sizeof(float)) : 0;
    P->off_hb = off;   off += (L.mode == 2 && !hidden_given) ? align_up(P->h_floats * sizeof(float)) : 0;
    P->off_xs = off;   off += xs_bytes ? xs_bytes - kAlign : 0;
    P->off_scal = off; off += xs_bytes ? kAlign : 0;
    P->off_blk = off;  off += blk_bytes;
    P->off_img = off;  off += P->attr_image ? img_bytes : 0;
    if (needed) *needed = off;
    // fused-kernel grid: ~one workgroup per CU, never more edge groups than 4-wave tile sets
    const int ns = L.K2P / GP_TN;
    int groups = num_cus_impl() / ns;
    if (groups < 1) groups = 1;
    const int64_t tiles_chunk = ((E + GP_TE - 1) / GP_TE + P->n_chunks - 1) / P->n_chunks;
    int64_t gcap = (tiles_chunk + GP_WAVES - 1) / GP_WAVES;
    // small graphs (MGKN levels): let a wave own as little as ONE destination node.  Its in-edges are a partial
    // tile (the matrix pipe idles anyway), but the per-node flush of Z - 32 KiB per node and slice - is what such a
    // launch spends its time on, and it is spread over the chip instead of a handful of waves
    const int64_t gcap_nodes = (npc + GP_WAVES - 1) / GP_WAVES;
    if (gcap < gcap_nodes) gcap = gcap_nodes;
    if (groups > gcap) groups = (int)(gcap < 1 ? 1 : gcap);
    P->n_groups = groups;
    return GPDE_OK;
}

// Which fused edge kernel serves a forward call -- ONE place, used by fwd_impl and by the query
// gpde_nnconv_fwd_kernel (bench.py / tests key profiles and expectations on the kernel symbol).
enum FusedKind { FK_GENERIC = 0, FK_V3 = 1, FK_V6 = 2 };
struct FusedChoice { FusedKind kind; bool g2f16; };
FusedChoice choose_fused(const GpdePackLayout& L, int mode, uint32_t flags, int64_t n_edges, int kt) {
    FusedChoice c{FK_GENERIC, false};
    if (mode != 1 || !(flags & GPDE_FWD_F16SPLIT)) return c;
    GpdeFusedArgs probe = gpde_fused_probe(L);
    probe.kt = kt;
    if (!gpde_fused_f16v3_supported(probe)) return c;
    c.kind = FK_V3;
    // f16-split aggregation inside the fused kernel: worth its three tiny pre-pass launches from a few ten
    // thousand edges on; GPDE_FWD_AGG_F16 / GPDE_FWD_AGG_F32 force it on / off
    c.g2f16 = !(flags & GPDE_FWD_AGG_F32) && n_edges > 0 && ((flags & GPDE_FWD_AGG_F16) || n_edges >= 32768);
    probe.xs = c.g2f16 ? (const unsigned*)(uintptr_t)8 : nullptr;      // "will be present"
    if (c.g2f16 && !(flags & GPDE_FWD_F16SPLIT_8WAVE) && gpde_fused_f16v6_supported(probe)) c.kind = FK_V6;
    return c;
}

bool attr_image_eligible(const GpdePackLayout& L, uint32_t flags, int64_t n_edges, int kt) {
    if ((flags & GPDE_FWD_NO_ATTR_IMAGE) || n_edges >= ((int64_t)1 << 31) - GP_QBLOCK) return false;
    if (choose_fused(L, L.mode, flags, n_edges, kt).kind != FK_V6) return false;
    return gpde_fused_f16v6_image_supported(gpde_fused_probe(L));
}

// Whether a forward call takes the per-edge last layer (fwd_impl's low in-degree branch) -- ONE place, used by fwd_impl
// and by the query gpde_nnconv_fwd_edge_path.  `hidden`: the last hidden activations are given (with their maximum:
// `hidden_absmax`); `mixed` / `kt`: the mixed and node-table forwards, which never take it.
bool takes_edge_path(const Plan& P, uint32_t flags, int64_t n_nodes, int64_t n_edges, bool hidden, bool hidden_absmax,
                     bool mixed, int kt) {
    const GpdePackLayout& L = P.L;
    bool store_ok = false;
    if (L.mode == 1 && L.k0 + 1 <= 8) store_ok = gpde_fused_store_supported(gpde_fused_probe(L));
    return ((flags & GPDE_FWD_F16SPLIT) || (hidden && hidden_absmax)) && !mixed && !kt && L.has_w3s && P.n_chunks == 1 &&
           n_edges >= 4096 && n_edges <= 4 * n_nodes && n_edges < ((int64_t)1 << 24) &&
           !(flags & GPDE_FWD_NO_EDGE_PATH) &&
           (hidden || (L.mode == 1 && store_ok)) &&   // H by a fused store kernel (its own support check: LDS limits, chunk parity)
           (size_t)(n_edges) * L.K2P + gpde_edge_messages_ws_floats(n_edges, GP_W * GP_W) <=
               (size_t)n_nodes * GP_W * L.K2P;
}

}  // namespace

int gpde_num_cus() { return num_cus_impl(); }

extern "C" const char* gpde_nnconv_fwd_kernel(int64_t n_edges, int n_layers, const int32_t* dims, uint32_t flags) {
    GpdePackLayout L;
    if (!dims || gpde_pack_layout(n_layers, dims, &L) != GPDE_OK) return "";
    switch (choose_fused(L, L.mode, flags, n_edges, 0).kind) {
        case FK_V6: return "gpde_fused_f16v6_kernel";
        case FK_V3: return "gpde_fused_f16v3_kernel";
        default: return "gpde_fused_kernel";
    }
}

extern "C" int gpde_nnconv_fwd_edge_path(int64_t n_nodes, int64_t n_edges, int n_layers, const int32_t* dims, uint32_t flags,
                                         size_t ws_bytes) {
    Plan P;
    if (!dims || n_nodes < 0 || n_edges < 0) { gpde_set_error("gpde_nnconv_fwd_edge_path: null/negative argument"); return GPDE_EINVAL; }
    int rc = make_plan(n_nodes, n_edges, n_layers, dims, ws_bytes, false, &P, nullptr, false, flags);
    if (rc != GPDE_OK) return rc;
    return takes_edge_path(P, flags, n_nodes, n_edges, false, false, false, 0) ? 1 : 0;
}

extern "C" int gpde_nnconv_fwd_attr_image(int64_t n_nodes, int64_t n_edges, int n_layers, const int32_t* dims, uint32_t flags,
                                          size_t ws_bytes, int32_t* n_chunks) {
    Plan P;
    if (!dims || n_nodes < 0 || n_edges < 0) { gpde_set_error("gpde_nnconv_fwd_attr_image: null/negative argument"); return GPDE_EINVAL; }
    int rc = make_plan(n_nodes, n_edges, n_layers, dims, ws_bytes, false, &P, nullptr, false, flags);
    if (rc != GPDE_OK) return rc;
    if (n_chunks) *n_chunks = P.n_chunks;
    return (P.attr_image && !takes_edge_path(P, flags, n_nodes, n_edges, false, false, false, 0)) ? 1 : 0;
}

extern "C" size_t gpde_nnconv_fwd_workspace_bytes(int64_t n_nodes, int64_t n_edges, int n_layers,
                                                  const int32_t* dims) {
    Plan P;
    size_t need = 0;
    if (!dims || n_nodes < 0 || n_edges < 0) return 0;
    if (make_plan(n_nodes, n_edges, n_layers, dims, 0, true, &P, &need) != GPDE_OK) return 0;
    return need + 2 * kAlign;
}

extern "C" int gpde_nnconv_fwd_plan(int64_t n_nodes, int64_t n_edges, int n_layers,
                                    const int32_t* dims, size_t ws_bytes, int32_t* n_chunks,
                                    int64_t* nodes_per_chunk, int32_t* fused_workgroups,
                                    int32_t* mode) {
    Plan P;
    if (!dims) { gpde_set_error("gpde_nnconv_fwd_plan: dims is null"); return GPDE_EINVAL; }
    int rc = make_plan(n_nodes, n_edges, n_layers, dims, ws_bytes, false, &P, nullptr);
    if (rc != GPDE_OK) return rc;
    if (n_chunks) *n_chunks = P.n_chunks;
    if (nodes_per_chunk) *nodes_per_chunk = P.nodes_per_chunk;
    if (fused_workgroups) *fused_workgroups = P.n_groups * (P.L.K2P / GP_TN);
    if (mode) *mode = P.L.mode;
    return GPDE_OK;
}

namespace {

// `hidden` != nullptr: the last hidden activations are given ([CSR slot][K2P], gpde_hidden_fwd); only the
// aggregation, the last Linear and update() run (gpde_nnconv_fwd_hidden)
// `kt` != 0: edge_attr is a NODE table [n_nodes][kt] and slot d of an edge's attribute is
// table[(sel[d] >> 8 ? dst : src)][sel[d] & 255] (gpde_nnconv_fwd_nodeattr)
// The arguments of fwd_impl by name.  A default means "not given"; `fwd_common` fills what every entry point has.
struct FwdArgs {
    const float* x = nullptr;
    int64_t n_nodes = 0, n_edges = 0;
    const int32_t *rowptr = nullptr, *src = nullptr, *dst = nullptr;
    int n_layers = 0;
    const int32_t* dims = nullptr;
    const void* packed = nullptr;
    const float *root = nullptr, *bias = nullptr;
    int aggr = 0;
    float* out = nullptr;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    hipStream_t stream = nullptr;
    // what an entry point may have
    const float* edge_attr = nullptr;       // [n_edges][k0] read through `perm`, or the node table when kt != 0
    const int32_t* perm = nullptr;
    uint32_t flags = 0;
    const float *hidden = nullptr, *hidden_absmax = nullptr;
    int64_t hidden_nodes = -1;              // -1: `hidden` covers every edge
    int kt = 0;                             // row stride of the node table
    const int* sel = nullptr;
    const float* residual = nullptr;
    int relu_out = 0;
    float* z_keep = nullptr;
};

FwdArgs fwd_common(const float* x, int64_t n_nodes, int64_t n_edges, const int32_t* rowptr, const int32_t* src, const int32_t* dst,
                   int n_layers, const int32_t* dims, const void* packed, const float* root, const float* bias, int aggr,
                   float* out, void* ws, size_t ws_bytes, void* stream) {
    FwdArgs a;
    a.x = x; a.n_nodes = n_nodes; a.n_edges = n_edges; a.rowptr = rowptr; a.src = src; a.dst = dst;
    a.n_layers = n_layers; a.dims = dims; a.packed = packed; a.root = root; a.bias = bias; a.aggr = aggr;
    a.out = out; a.ws = ws; a.ws_bytes = ws_bytes; a.stream = (hipStream_t)stream;
    return a;
}

int fwd_impl(const FwdArgs& a) {
    // hidden_nodes in [0, n_nodes): MIXED call (gpde_nnconv_fwd_mixed_keepz) -- `hidden` covers the in-edges of
    // nodes [0, hidden_nodes) only (a graph whose H does not fit memory, e.g. 391 GB at the 241^2 graph);
    // those nodes aggregate from it, the others run the fused kernel on edge_attr
    const bool mixed = a.hidden && a.hidden_nodes >= 0 && a.hidden_nodes < a.n_nodes;
    if (a.aggr != GPDE_AGGR_ADD && a.aggr != GPDE_AGGR_MEAN) {
        gpde_set_error("gpde_nnconv_fwd: aggr %d not implemented (add=0, mean=1)", a.aggr);
        return GPDE_EUNSUPPORTED;
    }
    if (a.n_nodes == 0) return GPDE_OK;
    if (!a.ws) { gpde_set_error("gpde_nnconv_fwd: workspace is null"); return GPDE_EWORKSPACE; }
    Plan P;
    int rc = make_plan(a.n_nodes, a.n_edges, a.n_layers, a.dims, a.ws_bytes, false, &P, nullptr, a.hidden != nullptr && !mixed,
                       a.flags, a.kt, a.hidden == nullptr);
    if (rc != GPDE_OK) return rc;
    const GpdePackLayout& L = P.L;
    const int mode = (a.hidden && !mixed) ? 2 : L.mode;
    if (mixed && L.mode != 1) { gpde_set_error("gpde_nnconv_fwd_mixed_keepz: built for 3-Linear kernel MLPs"); return GPDE_EUNSUPPORTED; }
    const float* pk = (const float*)a.packed;
    char* w = (char*)a.ws;
    w = (char*)(((uintptr_t)w + kAlign - 1) / kAlign * kAlign);
    float* part = (float*)(w + P.off_part);
    float* zbuf = (float*)(w + P.off_z);
    float* ha = (float*)(w + P.off_ha);
    float* hb = (float*)(w + P.off_hb);

    const float* hfinal = a.hidden;
    if (!a.hidden && L.mode == 2 && a.n_edges > 0) {   // (a mixed call has L.mode == 1)
        // front layers over all edges (CSR order), ping-pong between ha / hb
        const float* in = a.edge_attr;
        int ldx = L.k0, kin = L.k0;
        const int32_t* gather = a.perm;
        float* bufs[2] = {ha, hb};
        for (int l = 0; l < a.n_layers - 1; ++l) {
            GpdeDenseArgs d;
            d.X = in; d.ldx = ldx; d.kin = kin; d.gather = gather; d.row0 = 0;
            d.W = pk + L.off_front_w[l]; d.ldw = L.frontKP[l];
            d.b = pk + L.off_front_b[l];
            d.Y = bufs[l & 1]; d.KoutP = L.frontKP[l + 1];
            d.rows = (int)a.n_edges; d.relu = 1;
            rc = gpde_launch_dense(d, a.stream);
            if (rc != GPDE_OK) return rc;
            in = d.Y; ldx = kin = d.KoutP; gather = nullptr;
        }
        hfinal = in;
    }

    // ---- low in-degree graphs: the last Linear per EDGE (the reference's own association) --------------------------
    // The re-association of DESIGN.md §2 trades 8.4 MFLOP per edge for 8.4 MFLOP per NODE plus a 256 KiB Z round
    // trip per node - a loss when a node has two or three in-edges (MGKN-orthogonal Burgers: 8192 nodes, 16 k edges,
    // 2 x 2.1 GB of Z per call).  There W_e = W3 . h_e is formed tile by tile on the split-f16 GEMM and contracted
    // with x_j in its epilogue ([E][4096] never exists), messages are summed per destination in CSR order.
    const bool edge_path = !a.z_keep && takes_edge_path(P, a.flags, a.n_nodes, a.n_edges, a.hidden != nullptr,
                                                        a.hidden_absmax != nullptr, mixed, a.kt);
    if (edge_path) {
        float* Hbuf = zbuf;                                  // the Z region is free on this path
        float* ews = zbuf + (a.hidden ? 0 : (size_t)a.n_edges * L.K2P);
        const float* Hrows = a.hidden;
        if (!a.hidden) {
            ProfScope ps(GPDE_PROF_FUSED, a.stream);
            GpdeFusedArgs f{};
            f.attr = a.edge_attr; f.rowptr = a.rowptr; f.perm = a.perm;
            gpde_fused_set_pack(f, pk, L);
            f.hout = Hbuf; f.hmax_out = nullptr;
            f.nc0 = 0; f.nc1 = (int)a.n_nodes; f.e_chunk0 = 0;
            f.n_groups = gpde_fused_groups(L.K2P, gpde_group_cap_fwd(a.n_edges));
            if ((rc = gpde_launch_fused_store(f, a.stream)) != GPDE_OK) return rc;
            Hrows = Hbuf;
        }
        {
            ProfScope ps(GPDE_PROF_GEMM3, a.stream);
            rc = gpde_launch_edge_messages(Hrows, L.K2P, a.n_edges, pk + L.off_w3s, pk + L.off_ucol3, a.x, a.src, a.rowptr, a.n_nodes,
                                           ews, part, a.stream);
            if (rc != GPDE_OK) return rc;
        }
        GpdeEpilogueArgs e;
        e.part = part; e.x = a.x; e.rowptr = a.rowptr; e.src = a.src;
        e.b3 = pk + L.off_b3; e.root = a.root; e.bias = a.bias; e.out = a.out;
        e.nc0 = 0; e.nn = (int)a.n_nodes; e.splits = 1; e.aggr = a.aggr;
        e.residual = a.residual; e.relu_out = a.relu_out;
        ProfScope ps2(GPDE_PROF_EPILOGUE, a.stream);
        return gpde_launch_epilogue(e, a.stream);
    }

    const unsigned* xs = nullptr;
    const unsigned* scal = nullptr;
    GpdeAttrImage img{nullptr, nullptr, nullptr, nullptr};
    const FusedChoice fc = choose_fused(L, mode, a.flags, a.n_edges, a.kt);
    if (a.kt && fc.kind == FK_GENERIC) {
        gpde_set_error("gpde_nnconv_fwd_mixed_keepz (node_attr): built for 3-Linear kernel MLPs on the f16-split kernel only");
        return GPDE_EUNSUPPORTED;
    }
    if ((!a.hidden || mixed) && fc.g2f16) {
        ProfScope psp(GPDE_PROF_PREP, a.stream);
        rc = gpde_launch_g2_prep(a.x, a.n_nodes, a.edge_attr, a.n_edges, L.k0, pk + L.off_w1 + (size_t)L.K1P * 8,
                                 (unsigned*)(w + P.off_scal), (unsigned*)(w + P.off_xs), a.stream, a.kt, a.sel, a.src, a.dst);
        if (rc != GPDE_OK) return rc;
        xs = (const unsigned*)(w + P.off_xs);
        scal = (const unsigned*)(w + P.off_scal);
        if (P.attr_image && fc.kind == FK_V6) {
            // the f16v6 kernel's attribute operands, once per call instead of per tile, column slice and lane group
            img = gpde_attr_image_at(w + P.off_img, a.n_edges);
            rc = gpde_launch_attr_image(a.edge_attr, a.perm, a.n_edges, L.k0, pk + L.off_w1 + (size_t)L.K1P * 8, pk + L.off_fcol,
                                        img, a.stream, a.kt, a.sel, a.src, a.dst);
            if (rc != GPDE_OK) return rc;
        }
    }

    // hidden activations given together with their maximum: the streaming aggregation on split f16
    if (a.hidden && !mixed && a.hidden_absmax && a.n_edges >= 32768 && !(a.flags & GPDE_FWD_AGG_F32)) {
        rc = gpde_launch_g2_prep(a.x, a.n_nodes, nullptr, 0, 0, nullptr, (unsigned*)(w + P.off_scal),
                                 (unsigned*)(w + P.off_xs), a.stream);
        if (rc != GPDE_OK) return rc;
        xs = (const unsigned*)(w + P.off_xs);
        scal = (const unsigned*)(w + P.off_scal);
    }

    const int64_t hn = mixed ? a.hidden_nodes : (a.hidden ? a.n_nodes : 0);   // nodes served from `hidden`
    for (int64_t nc0 = 0, nc1 = 0; nc0 < a.n_nodes; nc0 = nc1) {
        const int64_t lim = nc0 < hn ? hn : a.n_nodes;                         // a chunk never straddles hn
        nc1 = (nc0 + P.nodes_per_chunk < lim) ? nc0 + P.nodes_per_chunk : lim;
        const bool from_h = nc0 < hn;
        const int nn = (int)(nc1 - nc0);
        const int splits = pick_splits(nn);
        if (a.n_edges > 0) {
            GpdeFusedArgs f{};
            f.x = a.x; f.attr = a.edge_attr; f.rowptr = a.rowptr; f.src = a.src; f.dst = a.dst; f.perm = a.perm;
            gpde_fused_set_pack(f, pk, L);
            float* zc = a.z_keep ? a.z_keep + (size_t)nc0 * GP_W * L.K2P : zbuf;
            f.hbuf = hfinal; f.zbuf = zc; f.xs = xs; f.scal = scal;
            f.kt = a.kt; f.hmax = (from_h && xs) ? (const unsigned*)a.hidden_absmax : nullptr;
            for (int d = 0; d < 8; ++d) f.sel[d] = (a.kt && a.sel) ? a.sel[d < L.k0 ? d : L.k0 - 1] : 0;
            f.nc0 = (int)nc0; f.nc1 = (int)nc1; f.e_chunk0 = 0; f.n_groups = P.n_groups;
            f.img_rec = img.rec; f.img_hi = img.hi; f.img_lo = img.lo; f.img_isc = img.isc;
            {
                ProfScope ps(GPDE_PROF_FUSED, a.stream);
                if (!from_h && fc.kind == FK_V6 && P.nblk_max && L.K2P / GP_TN <= 64 && !(a.flags & GPDE_FWD_STATIC_RANGES)) {
                    int32_t* blk = (int32_t*)(w + P.off_blk);
                    f.blk = blk; f.qn = blk + P.nblk_max + 1; f.qctr = (unsigned*)(blk + P.nblk_max + 2);
                    rc = gpde_launch_block_bounds(a.rowptr, (int)nc0, (int)nc1, P.nblk_max, blk, blk + P.nblk_max + 1,
                                                  (unsigned*)(blk + P.nblk_max + 2), L.K2P / GP_TN, a.stream);
                    if (rc != GPDE_OK) return rc;
                }
                if (from_h) rc = gpde_launch_zagg(f, a.stream);
                else if (fc.kind == FK_V6) rc = gpde_launch_fused_f16v6(f, a.stream);
                else if (fc.kind == FK_V3) rc = gpde_launch_fused_f16v3(f, a.stream);
                else rc = gpde_launch_fused(mode, (a.flags & GPDE_FWD_F16SPLIT) != 0 && mode == 1, f, a.stream);
            }
            if (rc != GPDE_OK) return rc;
            ProfScope ps1(GPDE_PROF_GEMM3, a.stream);
            GpdeGemm3Args g;
            g.zbuf = zc; g.w3q = pk + L.off_w3q; g.part = part; g.nn = nn; g.K2P = L.K2P;
            g.splits = splits; g.rowptr = a.rowptr; g.nc0 = (int)nc0;
            rc = gpde_launch_gemm3(g, a.stream);
            if (rc != GPDE_OK) return rc;
        }
        GpdeEpilogueArgs e;
        e.part = part; e.x = a.x; e.rowptr = a.rowptr; e.src = a.src;
        e.b3 = pk + L.off_b3; e.root = a.root; e.bias = a.bias; e.out = a.out;
        e.nc0 = (int)nc0; e.nn = nn; e.splits = splits; e.aggr = a.aggr;
        e.residual = a.residual; e.relu_out = a.relu_out;
        ProfScope ps2(GPDE_PROF_EPILOGUE, a.stream);
        rc = gpde_launch_epilogue(e, a.stream);
        if (rc != GPDE_OK) return rc;
    }
    return GPDE_OK;
}

}  // namespace

extern "C" int gpde_nnconv_fwd(const float* x, int64_t n_nodes, const float* edge_attr,
                               int64_t n_edges, const int32_t* rowptr, const int32_t* src,
                               const int32_t* dst, const int32_t* perm, int n_layers,
                               const int32_t* dims, const void* packed, const float* root,
                               const float* bias, int aggr, uint32_t flags, float* out, void* ws,
                               size_t ws_bytes, void* stream_) {
    if (n_nodes < 0 || n_edges < 0 || !dims || !packed || !rowptr || (n_nodes > 0 && (!x || !out)) ||
        (n_edges > 0 && (!edge_attr || !src || !dst || !perm))) {
        gpde_set_error("gpde_nnconv_fwd: null/negative argument");
        return GPDE_EINVAL;
    }
    FwdArgs a = fwd_common(x, n_nodes, n_edges, rowptr, src, dst, n_layers, dims, packed, root, bias, aggr, out, ws, ws_bytes, stream_);
    a.edge_attr = edge_attr; a.perm = perm; a.flags = flags;
    return fwd_impl(a);
}

// The general forward (round 5: the mixed, node-table and node-table + partial-H forwards folded into one): attributes from `edge_attr` +
// `perm` or from node data (`node_attr`: row f3; then edge_attr / perm are unused and may be NULL), optionally the part of the
// hidden activations that fits memory (`hidden`: rows of the in-edges of nodes [0, hidden_nodes); 0 = none), optionally Z kept
// for the backward (`z_keep`; NULL = none).
extern "C" int gpde_nnconv_fwd_mixed_keepz(const float* x, int64_t n_nodes, const float* edge_attr, const GpdeNodeAttr* node_attr,
                                           const float* hidden, const float* hidden_absmax, int64_t hidden_nodes, int64_t n_edges,
                                           const int32_t* rowptr, const int32_t* src, const int32_t* dst,
                                           const int32_t* perm, int n_layers, const int32_t* dims, const void* packed,
                                           const float* root, const float* bias, int aggr, uint32_t flags, float* z_keep,
                                           float* out, void* ws, size_t ws_bytes, void* stream_) {
    if (n_nodes < 0 || n_edges < 0 || !dims || !packed || !rowptr || (n_nodes > 0 && (!x || !out)) ||
        (n_edges > 0 && (!src || !dst || (!node_attr && (!edge_attr || !perm)))) || hidden_nodes < 0 || hidden_nodes > n_nodes ||
        (hidden_nodes > 0 && !hidden)) {
        gpde_set_error("gpde_nnconv_fwd_mixed_keepz: null/negative argument");
        return GPDE_EINVAL;
    }
    int kt = 0;
    int sel[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const float* attr = edge_attr;
    if (node_attr) {
        const GpdeNodeAttr* na = node_attr;
        if (!na->table || na->stride < 1 || na->n_slots != dims[0] || dims[0] < 1 || dims[0] > 7) {
            gpde_set_error("gpde_nnconv_fwd_mixed_keepz: GpdeNodeAttr must describe dims[0] = 1..7 slots of a node table");
            return GPDE_EINVAL;
        }
        for (int d = 0; d < 8; ++d) {
            sel[d] = na->sel[d < dims[0] ? d : dims[0] - 1];
            if ((sel[d] >> 8) < 0 || (sel[d] >> 8) > 1 || (sel[d] & 255) >= na->stride) {
                gpde_set_error("gpde_nnconv_fwd_mixed_keepz: GpdeNodeAttr.sel[%d] = 0x%x (endpoint << 8 | column, column < %d)", d, sel[d], na->stride);
                return GPDE_EINVAL;
            }
        }
        kt = na->stride;
        attr = na->table;
        perm = nullptr;
    }
    FwdArgs a = fwd_common(x, n_nodes, n_edges, rowptr, src, dst, n_layers, dims, packed, root, bias, aggr, out, ws, ws_bytes, stream_);
    a.edge_attr = attr; a.perm = perm; a.flags = flags; a.kt = kt; a.sel = kt ? sel : nullptr; a.z_keep = z_keep;
    if (hidden_nodes != 0) { a.hidden = hidden; a.hidden_absmax = hidden_absmax; a.hidden_nodes = hidden_nodes; }
    return fwd_impl(a);
}

extern "C" int gpde_nnconv_fwd_hidden(const float* x, int64_t n_nodes, const float* hidden,
                                      const float* hidden_absmax, int64_t n_edges, const int32_t* rowptr, const int32_t* src,
                                      const int32_t* dst, int n_layers, const int32_t* dims,
                                      const void* packed, const float* root, const float* bias,
                                      int aggr, float* out, void* ws, size_t ws_bytes, void* stream_) {
    if (n_nodes < 0 || n_edges < 0 || !dims || !packed || !rowptr || (n_nodes > 0 && (!x || !out)) ||
        (n_edges > 0 && (!hidden || !src || !dst))) {
        gpde_set_error("gpde_nnconv_fwd_hidden: null/negative argument");
        return GPDE_EINVAL;
    }
    FwdArgs a = fwd_common(x, n_nodes, n_edges, rowptr, src, dst, n_layers, dims, packed, root, bias, aggr, out, ws, ws_bytes, stream_);
    a.hidden = hidden; a.hidden_absmax = hidden_absmax;
    return fwd_impl(a);
}

extern "C" int gpde_nnconv_fwd_act(const float* x, int64_t n_nodes, const float* edge_attr, int64_t n_edges,
                                   const int32_t* rowptr, const int32_t* src, const int32_t* dst, const int32_t* perm,
                                   int n_layers, const int32_t* dims, const void* packed, const float* root,
                                   const float* bias, int aggr, uint32_t flags, const float* residual, int relu_out,
                                   float* out, void* ws, size_t ws_bytes, void* stream_) {
    if (n_nodes < 0 || n_edges < 0 || !dims || !packed || !rowptr || (n_nodes > 0 && (!x || !out)) ||
        (n_edges > 0 && (!edge_attr || !src || !dst || !perm)) || (residual && residual == out)) {
        gpde_set_error("gpde_nnconv_fwd_act: null/negative argument (or residual aliases out)");
        return GPDE_EINVAL;
    }
    FwdArgs a = fwd_common(x, n_nodes, n_edges, rowptr, src, dst, n_layers, dims, packed, root, bias, aggr, out, ws, ws_bytes, stream_);
    a.edge_attr = edge_attr; a.perm = perm; a.flags = flags; a.residual = residual; a.relu_out = relu_out;
    return fwd_impl(a);
}

extern "C" int gpde_nnconv_fwd_hidden_act(const float* x, int64_t n_nodes, const float* hidden, const float* hidden_absmax,
                                          int64_t n_edges, const int32_t* rowptr, const int32_t* src, const int32_t* dst,
                                          int n_layers, const int32_t* dims, const void* packed, const float* root,
                                          const float* bias, int aggr, const float* residual, int relu_out, float* out,
                                          void* ws, size_t ws_bytes, void* stream_) {
    if (n_nodes < 0 || n_edges < 0 || !dims || !packed || !rowptr || (n_nodes > 0 && (!x || !out)) ||
        (n_edges > 0 && (!hidden || !src || !dst)) || (residual && residual == out)) {
        gpde_set_error("gpde_nnconv_fwd_hidden_act: null/negative argument (or residual aliases out)");
        return GPDE_EINVAL;
    }
    FwdArgs a = fwd_common(x, n_nodes, n_edges, rowptr, src, dst, n_layers, dims, packed, root, bias, aggr, out, ws, ws_bytes, stream_);
    a.hidden = hidden; a.hidden_absmax = hidden_absmax; a.residual = residual; a.relu_out = relu_out;
    return fwd_impl(a);
}

extern "C" int gpde_nnconv_fwd_keepz(const float* x, int64_t n_nodes, const float* edge_attr, const float* hidden,
                                     const float* hidden_absmax, int64_t n_edges, const int32_t* rowptr, const int32_t* src,
                                     const int32_t* dst, const int32_t* perm, int n_layers, const int32_t* dims,
                                     const void* packed, const float* root, const float* bias, int aggr, uint32_t flags,
                                     float* z_keep, float* out, void* ws, size_t ws_bytes, void* stream_) {
    if (n_nodes < 0 || n_edges < 0 || !dims || !packed || !rowptr || (n_nodes > 0 && (!x || !out || !z_keep)) ||
        (n_edges > 0 && (!src || !dst || (!hidden && (!edge_attr || !perm))))) {
        gpde_set_error("gpde_nnconv_fwd_keepz: null/negative argument");
        return GPDE_EINVAL;
    }
    FwdArgs a = fwd_common(x, n_nodes, n_edges, rowptr, src, dst, n_layers, dims, packed, root, bias, aggr, out, ws, ws_bytes, stream_);
    a.z_keep = z_keep;
    if (hidden) { a.hidden = hidden; a.hidden_absmax = hidden_absmax; }      // (attributes, perm and flags are not read)
    else { a.edge_attr = edge_attr; a.perm = perm; a.flags = flags; }
    return fwd_impl(a);
}

extern "C" int gpde_profile_begin(void) {
    for (auto& p : g_prof) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    g_prof.clear();
    g_prof_on = true;
    return GPDE_OK;
}

extern "C" int gpde_profile_end_kinds(double* ms_by_kind, int32_t* launches_by_kind) {
    g_prof_on = false;
    for (int k = 0; k < GPDE_PROF_KINDS; ++k) {
        if (ms_by_kind) ms_by_kind[k] = 0.0;
        if (launches_by_kind) launches_by_kind[k] = 0;
    }
    for (auto& p : g_prof) {
        float ms = 0.f;
        GP_HIP_CHECK(hipEventSynchronize(p.b));
        GP_HIP_CHECK(hipEventElapsedTime(&ms, p.a, p.b));
        const int k = (p.kind >= 0 && p.kind < GPDE_PROF_KINDS) ? p.kind : GPDE_PROF_KINDS - 1;
        if (ms_by_kind) ms_by_kind[k] += ms;
        if (launches_by_kind) launches_by_kind[k] += 1;
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    g_prof.clear();
    return GPDE_OK;
}

