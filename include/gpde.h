/*
 * gpde.h — C ABI of libgpde.so: the MI355X (gfx950) edge-conditioned graph convolution
 * (NNConv) hot path of neuraloperator/graph-pde.
 *
 * The reference has no FFI: the path sits behind a Python `torch.nn.Module`
 * (`nn_conv.NNConv_old`, /root/reference/graph-neural-operator/nn_conv.py:197-286, and
 * `torch_geometric.nn.NNConv`) whose `forward(x, edge_index, edge_attr)` dispatches stock
 * PyTorch / torch_scatter kernels.  These entry points are what a binding for that path binds
 * (INTEGRATION.md shows the ctypes stub); each one names the reference code it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless marked "host"; buffers are row-major, contiguous,
 *    float32 / int32 / int64 exactly as named; `edge_index` alone carries explicit strides;
 *  - calls are asynchronous on `stream` (a hipStream_t passed as void*; NULL = the null stream),
 *    re-entrant, never synchronise, never allocate: the caller supplies the workspace
 *    (query with the *_workspace_bytes functions);
 *  - return value: GPDE_OK or a negative GPDE_E* code; gpde_last_error() (thread-local) gives
 *    the message.  Nothing throws across the ABI.
 */
#ifndef GPDE_H
#define GPDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPDE_VERSION 101 /* 0.1.1: + gpde_nnconv_bwd_edgeweights_acc */
/* gpde_version() of a developer build carries one of these on top of GPDE_VERSION: an ABLATION build has part of the arithmetic
 * compiled out (timing experiments; its results are WRONG and a binding must refuse it), an INSTRUMENTED build carries
 * clock probes (results correct). */
#define GPDE_VERSION_ABLATION 0x10000
#define GPDE_VERSION_INSTRUMENTED 0x20000

/* libgpde.so is built with -fvisibility=hidden: the entry points declared here are its ONLY dynamic symbols (internal
 * launchers and kernels stay out of the dynamic symbol table; tests/test_abi.py diffs `nm -D` against this header). */
#define GPDE_API __attribute__((visibility("default")))

enum {
    GPDE_OK = 0,
    GPDE_EINVAL = -1,       /* bad argument (null pointer, negative size, ...) */
    GPDE_EUNSUPPORTED = -2, /* shape outside what the kernels implement */
    GPDE_EWORKSPACE = -3,   /* workspace too small */
    GPDE_EHIP = -4          /* a HIP runtime call / kernel launch failed */
};

enum { GPDE_AGGR_ADD = 0, GPDE_AGGR_MEAN = 1,
       GPDE_AGGR_MAX = 2 /* gpde_nnconv_fwd_edgeweights_group only: 'max' cannot use the re-associated contraction */ };

/* gpde_nnconv_fwd flags */
enum {
    GPDE_FWD_DEFAULT = 0,  /* every contraction on v_mfma_f32_32x32x2_f32: exact fp32 (fmaf chains) */
    GPDE_FWD_F16SPLIT = 1, /* hidden k1 x k2 layer on f16 MFMA with two-term operand splitting
                              (x = hi + lo, 3 MFMAs, fp32 accumulate; per-product error < 2^-21,
                              DESIGN.md §3b); ignored for kernels without a hidden GEMM */
    GPDE_FWD_F16SPLIT_8WAVE = 2, /* with F16SPLIT: force the 8-wave kernel (gpde_fused_f16v3_kernel: the path of small
                                    graphs, node-table attributes and gpde_hidden_fwd) where the default would be the
                                    one-wave-per-SIMD kernel gpde_fused_f16v6_kernel (A/B, parity tests) */
    GPDE_FWD_STATIC_RANGES = 4,  /* gpde_fused_f16v6_kernel: one contiguous edge range per wave instead of the block work queue
                                    (A/B of the x_j gather locality, parity tests) */
    GPDE_FWD_AGG_F16 = 16,       /* with F16SPLIT: aggregation x_j (x) h_e on split-f16 MFMA too, also for small
                                    graphs (default: from 32768 edges on; three tiny pre-pass launches) */
    GPDE_FWD_AGG_F32 = 32,       /* with F16SPLIT: keep the aggregation on fp32 MFMA (A/B) */
    GPDE_FWD_NO_EDGE_PATH = 64,  /* never take the per-edge last layer of low in-degree graphs (mean in-degree <= 4,
                                  * >= 4096 edges, k2 >= 256: W_e = W3 . h_e on the split-f16 GEMM, contracted with x_j
                                  * in its epilogue) - A/B against the re-associated path */
    GPDE_FWD_NO_ATTR_IMAGE = 128 /* gpde_fused_f16v6_kernel: form the attribute operands of the first hidden layer in every
                                  * tile's prologue instead of reading the per-call attribute operand image (A/B, parity
                                  * tests; same bytes out) */
};

#define GPDE_MAX_LAYERS 8
#define GPDE_WIDTH 64 /* node-feature width (in_channels == out_channels) the kernels are built for */

/* Edge attributes described by NODE data instead of an [E][k0] tensor (details at gpde_nnconv_fwd_mixed_keepz):
 * slot d of edge (j -> i) is table[(sel[d] >> 8 ? i : j) * stride + (sel[d] & 255)].  A HOST struct; every entry point that takes
 * `edge_attr` + `perm` also takes a `const GpdeNodeAttr* node_attr` (NULL = the tensor) - round 5 folded the `_na` twins into it. */
typedef struct GpdeNodeAttr {
    const float* table;   /* device [n_nodes][stride] */
    int32_t stride;
    int32_t n_slots;      /* = dims[0], 1..7 */
    int32_t sel[8];       /* slot d: endpoint << 8 | column (endpoint 0 = source j, 1 = target i) */
} GpdeNodeAttr;

GPDE_API int gpde_version(void);
GPDE_API const char* gpde_last_error(void);
/* The library's developer / A-B switches (GPDE_BWD_*, GPDE_EDGE_BWD, GPDE_DEBUG_SKEW_US, ...: INTEGRATION.md) are environment
 * variables read ONCE, at the first native call of the process - no launch path calls getenv().  This re-reads them (test
 * suites and A/B scripts that flip a switch inside one process). */
GPDE_API int gpde_reload_switches(void);

/* ---------------------------------------------------------------------------------------------
 * Destination-sorted CSR of a COO edge list.
 * Replaces what `MessagePassing.propagate` does implicitly on every call: the gather by
 * `edge_index[0]` and the scatter by `edge_index[1]` (call site nn_conv.py:271; PyG semantics in
 * SURVEY.md Appendix B).  The sort is STABLE: within one destination the edges keep their input
 * order, so the per-destination summation order is fixed run to run.
 *
 *   edge_index : int64, element (r, e) at edge_index[r*stride_row + e*stride_col]
 *                (row 0 = source j, row 1 = target i; may be a strided view)
 *   rowptr[N+1]: in-edges of node i are CSR slots rowptr[i] .. rowptr[i+1]-1
 *   src[E], dst[E] : source / target node of each CSR slot;  perm[E] : its original edge id
 *   n_bad      : int32 device word, receives the number of edges with an endpoint outside [0,N)
 *                (those edges are dropped from the CSR; the reference would raise IndexError)
 */
GPDE_API size_t gpde_csr_workspace_bytes(int64_t n_edges, int64_t n_nodes);
GPDE_API int gpde_csr_from_coo(const int64_t* edge_index, int64_t stride_row, int64_t stride_col,
                      int64_t n_edges, int64_t n_nodes, int32_t* rowptr, int32_t* src,
                      int32_t* dst, int32_t* perm, int32_t* n_bad, void* ws, size_t ws_bytes,
                      void* stream);
/* The same for a RECTANGULAR edge list - sources j in [0, n_src), destinations i in [0, n_dst), two different node sets (PyG's
 * `propagate(edge_index, size=(n_src, n_dst), x=(x_src, x_dst))`): rowptr has n_dst + 1 entries, src[] indexes the n_src sources.
 * Row 0 of edge_index is checked against [0, n_src) and row 1 against [0, n_dst); n_bad counts the edges that violate either.
 * The same stable order; with n_src == n_dst the four arrays are those of gpde_csr_from_coo bit for bit (one body serves both).
 * Workspace: gpde_csr_workspace_bytes(n_edges, max(n_src, n_dst)).  An addition to the ABI: GPDE_VERSION is unchanged. */
GPDE_API int gpde_csr_from_coo2(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t n_edges,
                       int64_t n_src, int64_t n_dst, int32_t* rowptr, int32_t* src, int32_t* dst, int32_t* perm,
                       int32_t* n_bad, void* ws, size_t ws_bytes, void* stream);
/* out[s][0..k) = rows[perm[s]][0..k) for the n CSR slots: a per-edge tensor (edge_attr [E][k0], the `pseudo` of
 * nn_conv.py:271) laid out by CSR slot, once per (graph, tensor), so that the fused kernels stream it instead of chasing
 * perm (8 column slices x one cache line per edge otherwise).  Same values: results are bit-identical. */
GPDE_API int gpde_gather_rows(const float* rows, int k, const int32_t* perm, int64_t n, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Kernel-MLP weights, repacked once per parameter update into MFMA-tile order.
 * Replaces nothing arithmetic: it is the layout step for `DenseNet`'s `nn.Linear` weights
 * (/root/reference/graph-neural-operator/utilities.py:201-227; torch layout weight[out][in]).
 *
 *   n_layers      : number of Linear layers (>= 2); ReLU between them, none after the last
 *   dims[n_layers+1] (host): k0, k1, ..., 4096 (= GPDE_WIDTH^2)
 *   W[l], b[l] (host arrays of device pointers): weight [dims[l+1]][dims[l]], bias [dims[l+1]]
 *                (b[l] may be NULL = no bias)
 *   packed        : device buffer of gpde_mlp_pack_bytes() bytes
 */
GPDE_API size_t gpde_mlp_pack_bytes(int n_layers, const int32_t* dims);
GPDE_API int gpde_mlp_pack(int n_layers, const int32_t* dims, const float* const* W,
                  const float* const* b, void* packed, size_t packed_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused NNConv forward:  out[i] = aggr_{e: j->i} ( x[j] . reshape(mlp(edge_attr[e]), [64,64]) )
 *                                 + x[i] . root + bias
 * Replaces NNConv_old.forward / message / update (nn_conv.py:267-282), DenseNet.forward
 * (utilities.py:223-227) and PyG's gather + scatter-add/mean in one pass
 * that never materialises the [E,4096] per-edge weight tensor.
 *
 *   x [N][64], edge_attr [E][k0] in ORIGINAL edge order (gathered through perm),
 *   rowptr/src/dst/perm from gpde_csr_from_coo, packed from gpde_mlp_pack (same n_layers/dims),
 *   root [64][64] or NULL, bias [64] or NULL, aggr = GPDE_AGGR_ADD | GPDE_AGGR_MEAN
 *   (mean = sum / max(in_degree,1): zero in-degree rows receive only root/bias terms),
 *   out [N][64] (fully overwritten).
 *   ws: gpde_nnconv_fwd_workspace_bytes() is the recommended size; any size that holds one
 *   64-node tile works (more workspace = more destination nodes per launch), else GPDE_EWORKSPACE.
 */
GPDE_API size_t gpde_nnconv_fwd_workspace_bytes(int64_t n_nodes, int64_t n_edges, int n_layers,
                                       const int32_t* dims);
GPDE_API int gpde_nnconv_fwd(const float* x, int64_t n_nodes, const float* edge_attr, int64_t n_edges,
                    const int32_t* rowptr, const int32_t* src, const int32_t* dst,
                    const int32_t* perm, int n_layers, const int32_t* dims, const void* packed,
                    const float* root, const float* bias, int aggr, uint32_t flags, float* out,
                    void* ws, size_t ws_bytes, void* stream);

/* gpde_nnconv_fwd / gpde_nnconv_fwd_hidden with the callers' elementwise glue fused into the last kernel
 * (opt-in, the module surface does not change):
 *     out = act(residual + NNConv(x))        residual [N][64] or NULL (may alias x, must not alias out),
 *                                            relu_out != 0: act = max(., 0), else identity
 * - `F.relu(x + conv(x, ...))` of the MGKN V-cycles (MGKN_general_darcy2d.py:79-80,89-90;
 * MGKN_orthogonal_burgers1d.py:74-82) and `F.relu(conv(...))` of KernelNN.forward (UAI1_full_resolution.py:30). */
GPDE_API int gpde_nnconv_fwd_act(const float* x, int64_t n_nodes, const float* edge_attr, int64_t n_edges,
                        const int32_t* rowptr, const int32_t* src, const int32_t* dst, const int32_t* perm,
                        int n_layers, const int32_t* dims, const void* packed, const float* root,
                        const float* bias, int aggr, uint32_t flags, const float* residual, int relu_out,
                        float* out, void* ws, size_t ws_bytes, void* stream);
GPDE_API int gpde_nnconv_fwd_hidden_act(const float* x, int64_t n_nodes, const float* hidden, const float* hidden_absmax,
                               int64_t n_edges, const int32_t* rowptr, const int32_t* src, const int32_t* dst,
                               int n_layers, const int32_t* dims, const void* packed, const float* root,
                               const float* bias, int aggr, const float* residual, int relu_out, float* out,
                               void* ws, size_t ws_bytes, void* stream);

/* Launch plan gpde_nnconv_fwd will follow for these sizes and this workspace (host-side query, no
 * device work): number of destination-node chunks, nodes per chunk, workgroups of the fused
 * kernel per chunk, and which fused variant runs (0: one hidden layer, 1: two hidden layers with
 * the first generated on the fly, 2: hidden activations precomputed by dense front layers). */
GPDE_API int gpde_nnconv_fwd_plan(int64_t n_nodes, int64_t n_edges, int n_layers, const int32_t* dims,
                         size_t ws_bytes, int32_t* n_chunks, int64_t* nodes_per_chunk,
                         int32_t* fused_workgroups, int32_t* mode);

/* Symbol (without template arguments) of the fused edge kernel gpde_nnconv_fwd launches for a graph of
 * `n_edges` edges, this kernel MLP and these flags: "gpde_fused_f16v6_kernel" (one wave per SIMD, 64 x 128
 * wave tile; GPDE_FWD_F16SPLIT from 32768 edges on), "gpde_fused_f16v3_kernel" (8 waves; smaller graphs,
 * GPDE_FWD_F16SPLIT_8WAVE) or "gpde_fused_kernel" (fp32 MFMA; 2-Linear and >= 4-Linear kernels).  Host-side
 * query, no device work; static storage.  bench.py keys its rocprofv3 / PMC records on this name.
 * It names the kernel of the RE-ASSOCIATED path; a low in-degree graph (mean in-degree <= 4, >= 4096 edges, k2 >= 256,
 * one node chunk: DESIGN.md §3e) runs the store variant of the same kernel family plus gpde_gemm_f16s_nt_kernel instead -
 * whether it does depends on the node count and the workspace, which this query does not see. */
GPDE_API const char* gpde_nnconv_fwd_kernel(int64_t n_edges, int n_layers, const int32_t* dims, uint32_t flags);

/* 1 when gpde_nnconv_fwd with these sizes, kernel MLP, flags and `ws_bytes` of workspace takes the per-edge last layer
 * (W_e = W3 . h_e per edge, gpde_gemm_f16s_nt_kernel) instead of the re-associated path gpde_nnconv_fwd_kernel names; 0 when
 * it does not; < 0 (GpdeStatus) on invalid arguments or a workspace too small for the call.  Host only, no device work. */
GPDE_API int gpde_nnconv_fwd_edge_path(int64_t n_nodes, int64_t n_edges, int n_layers, const int32_t* dims, uint32_t flags,
                                       size_t ws_bytes);

/* 1 when that call runs gpde_fused_f16v6_kernel on the attribute operand image (36 bytes per edge of the workspace, built
 * once per call: gpde_nnconv_fwd_workspace_bytes counts them wherever the default flags choose that kernel; a smaller
 * workspace, GPDE_FWD_NO_ATTR_IMAGE or k1 above 1152 keep the operands in the kernel's tile prologue); 0 when it does
 * not; < 0 as above.  `n_chunks` (nullable): the node chunks of the call's plan under these flags.  Host only. */
GPDE_API int gpde_nnconv_fwd_attr_image(int64_t n_nodes, int64_t n_edges, int n_layers, const int32_t* dims, uint32_t flags,
                                        size_t ws_bytes, int32_t* n_chunks);

/* ---------------------------------------------------------------------------------------------
 * Backward of the fused NNConv (what autograd computes through nn_conv.py:267-282,
 * utilities.py:223-227 and PyG's gather/scatter on `loss.backward()`,
 * UAI1_full_resolution.py:266).  Given grad_out = dL/d(out) [N][64] it writes (overwrites)
 *   grad_x [N][64], grad_W[l] [dims[l+1]][dims[l]], grad_b[l] [dims[l+1]] (torch layouts; entries
 *   or whole arrays may be NULL to skip), grad_root [64][64], grad_bias [64] (NULL to skip).
 * W, b, grad_W, grad_b are HOST arrays of device pointers; rowptr_host is a HOST copy of rowptr
 * (the edge chunks are planned on the host).  Hidden activations are recomputed per node-aligned
 * chunk of edges; nothing from the forward needs to be saved (z_saved is an option, below).  fp32-class
 * arithmetic throughout (fp32 MFMA; split-f16 MFMA at < 2^-21 per product where DESIGN.md §6b says so). */
GPDE_API size_t gpde_nnconv_bwd_workspace_bytes(int64_t n_nodes, int64_t n_edges, int n_layers,
                                       const int32_t* dims);
/* The workspace with which the backward runs ALL edges and nodes as ONE chunk (the call above caps its answer at ~26 GB and
 * the backward then walks node-aligned chunks of ~640 k edges at k = 1024).  Any size in between is accepted and gives
 * proportionally fewer chunks; fewer chunks are faster (s=121, 5.9 M edges: 152 ms with 10 chunks, 147 ms with one) - a
 * caller with memory to spare may pass up to this many bytes (ops.py: when it is below GPDE_BWD_WS_FRACTION of the free device
 * memory). */
GPDE_API size_t gpde_nnconv_bwd_workspace_bytes_one_chunk(int64_t n_nodes, int64_t n_edges, int n_layers,
                                                 const int32_t* dims);
/* The node chunking gpde_nnconv_bwd (n_defer = 0) or gpde_nnconv_bwd_deferred (n_defer = L) plans for these sizes and `ws_bytes` of
 * workspace: edges and nodes per node-aligned chunk (a chunk ends at the last node whose in-edges still fit both).  h_given: the last
 * hidden activations of every edge come from the caller (gpde_nnconv_bwd's `hidden` + attribute source form).  Host only, no device
 * work; GPDE_EWORKSPACE when the workspace is too small. */
GPDE_API int gpde_nnconv_bwd_plan(int64_t n_nodes, int64_t n_edges, int n_layers, const int32_t* dims, size_t ws_bytes,
                                  int n_defer, int h_given, int64_t* edges_per_chunk, int64_t* nodes_per_chunk);
enum { GPDE_BWD_ACCUMULATE_GRAD_HIDDEN = 1 /* gpde_nnconv_bwd `flags`, `hidden` form: grad_hidden += dL/dU instead of = (see below) */ };
GPDE_API int gpde_nnconv_bwd(const float* x, int64_t n_nodes, const float* edge_attr, const GpdeNodeAttr* node_attr,
                    const float* hidden, int64_t n_edges, const int32_t* rowptr, const int32_t* src, const int32_t* dst,
                    const int32_t* perm, const int32_t* rowptr_host, const int32_t* src_rowptr, const int32_t* src_slots,
                    int n_layers, const int32_t* dims, const float* const* W, const float* const* b, const float* root,
                    int aggr, const float* grad_out, const float* z_saved, float* grad_x, float* grad_hidden,
                    float* grad_edge_attr, float* const* grad_W, float* const* grad_b, float* grad_root,
                    float* grad_bias, uint32_t flags, void* ws, size_t ws_bytes, void* stream);
/* ^ ONE backward entry point for every form of the operator (round 5 folded seven: the plain, source-ordered, kept-Z,
 *   given-hidden, edge-attribute-gradient and node-table calls of rounds 1-4 were this call with some arguments fixed):
 *   attribute source   edge_attr + perm (tensor, caller's edge order) | node_attr (node data) | hidden (the last hidden
 *                      activations given, [CSR slot][K2P], e.g. from gpde_hidden_fwd: only x, the LAST Linear (W / b / grad_W /
 *                      grad_b carry their last entries), root and bias are differentiated, and dL/dU of the last hidden layer
 *                      is written to grad_hidden [CSR slot][K2P] for gpde_hidden_bwd).  Exactly one of the three - except:
 *   hidden + an attribute source, grad_hidden == NULL   the FULL backward (every layer differentiated) with the last hidden
 *                      activations KEPT BY THE FORWARD (gpde_hidden_fwd, then gpde_nnconv_fwd_keepz on them): read where they would
 *                      be recomputed - the K loop of the hidden layer runs once per training step instead of twice, for 4 KiB
 *                      per edge of memory between forward and backward (the host mirror keeps them when they fit, GPDE_SAVE_H_GB).
 *   src_rowptr, src_slots  nullable: the CSR slots regrouped by source node (gpde_csr_source_order) - grad_x is then summed per
 *                      source in slot order, bit-reproducible and independent of the chunking; NULL: fp32 atomics.
 *   z_saved            nullable: the Z buffer of gpde_nnconv_fwd_keepz / _mixed_keepz - dW_3 is taken from it.
 *   flags              0, or GPDE_BWD_ACCUMULATE_GRAD_HIDDEN (the `hidden` form): dL/dU is ADDED to grad_hidden.  A module applied
 *                      `depth` times on shared hidden activations (UAI1_full_resolution.py:29-30) sums the dL/dU of its applications
 *                      before gpde_hidden_bwd: the first application's backward writes the tensor, the others add to it in the per-edge
 *                      kernel, in call order - the additions autograd would make with `depth` [E][K2P] tensors, without the tensors
 *                      (built into the split-f16 per-edge kernel; GPDE_EUNSUPPORTED elsewhere).
 *   grad_hidden        the `hidden` form only.   grad_edge_attr  nullable, tensor form with <= 8 slots only: dL/d edge_attr
 *                      [E][k0] in the caller's edge order (what autograd hands `pseudo`, nn_conv.py:273-275; no reference
 *                      script asks for it).
 * On grad_x: without the source order dx_j is accumulated over the out-edges of j by fp32 atomics (run-to-run differences at
 * the 1e-7 level, like the reference's index_select backward on a GPU); with it the per-edge contributions are written out
 * and summed per source in ascending slot order by one owner per element.  Weight gradients are ordered either way. */
/* src_slots = CSR slots 0..E-1 stably sorted by their source node, src_rowptr[j] = first position of source j;
 * `src` is the array gpde_csr_from_coo wrote; workspace: gpde_csr_workspace_bytes(n_edges, n_nodes).
 * `n_nodes` counts the SOURCE nodes: for a rectangular graph (gpde_csr_from_coo2) pass n_src - src_rowptr then has n_src + 1
 * entries, which is what the *_bip backward entry points take. */
GPDE_API int gpde_csr_source_order(const int32_t* src, int64_t n_edges, int64_t n_nodes, int32_t* src_rowptr,
                          int32_t* src_slots, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-depth reuse of the kernel MLP.  The reference applies ONE NNConv
 * module `depth` times per forward with the same edge_attr and the same weights
 * (UAI1_full_resolution.py:29-30 `for k in range(self.depth): x = F.relu(self.conv1(x, ...))`;
 * MGKN_general_darcy2d.py:76-90, MGKN_orthogonal_burgers1d.py:65-82), so the hidden activation
 *   H_e = relu(L_{n-1}(... relu(L_1(edge_attr_e))))     (DenseNet.forward, utilities.py:223-227,
 *                                                         all but the last Linear)
 * is identical in every one of those calls.  The operator splits into
 *   gpde_hidden_fwd:         edge_attr -> H            [E][K2P] fp32, rows in CSR (destination-sorted)
 *                            order, K2P = dims[n_layers-1] rounded up to 128, padding columns zero
 *   gpde_nnconv_fwd_hidden:  (x, H) -> out             aggregation + last Linear + update()
 * and, for training, their backward halves
 *   gpde_nnconv_bwd(hidden): grad_out -> grad_x, grad of the last Linear / root / bias, and
 *                            grad_hidden = dL/dU of the last hidden layer (already multiplied by the
 *                            ReLU mask H > 0), [E][K2P], overwritten
 *   gpde_hidden_bwd:         grad_hidden (summed over the `depth` uses by the caller's autograd)
 *                            -> gradients of the hidden Linear layers 0 .. n_layers-2 (grad_W / grad_b
 *                            entries of the last layer are ignored)
 * so the k1 x k2 layer (94 % of the FLOPs) and its backward run once per step instead of `depth`
 * times.  The caller owns H (E * K2P * 4 bytes) and decides whether it fits.
 *
 * gpde_hidden_fwd: with flags & GPDE_FWD_F16SPLIT, `packed` (gpde_mlp_pack) and a 3-Linear MLP the
 * fused f16-split kernel computes H (same arithmetic as gpde_nnconv_fwd); otherwise the layers run
 * as fp32-MFMA GEMMs over chunks of edges and W, b (HOST arrays of device pointers, torch layouts)
 * and ws (gpde_hidden_workspace_bytes) are required.  Workspaces: gpde_nnconv_fwd_hidden ->
 * gpde_nnconv_fwd_workspace_bytes; gpde_nnconv_bwd -> gpde_nnconv_bwd_workspace_bytes; gpde_hidden_bwd:
 * gpde_nnconv_bwd_workspace_bytes(0, E, ...).
 * hidden_absmax (nullable, one device float): gpde_hidden_fwd records max |H| there when its fused
 * path computed H (the general path leaves 0: the value is then NOT a maximum and must not be
 * passed on).  Given back to gpde_nnconv_fwd_hidden it lets the aggregation run on split-f16 MFMA
 * from 32768 edges on; NULL: fp32 MFMA. */
GPDE_API size_t gpde_hidden_workspace_bytes(int64_t n_edges, int n_layers, const int32_t* dims);
GPDE_API int gpde_hidden_fwd(const float* edge_attr, const GpdeNodeAttr* node_attr, int64_t n_edges, const int32_t* rowptr,
                    int64_t n_nodes, const int32_t* perm, const int32_t* src, const int32_t* dst, int n_layers,
                    const int32_t* dims, const void* packed, const float* const* W, const float* const* b, uint32_t flags,
                    float* hidden, float* hidden_absmax, void* ws, size_t ws_bytes, void* stream);
/* ^ node_attr != NULL: attributes from node data (src / dst required, edge_attr / perm / W / b / ws unused; 3-Linear kernel MLPs of
 *   >= 8 k1 chunks on GPDE_FWD_F16SPLIT); else src / dst may be NULL. */
GPDE_API int gpde_nnconv_fwd_hidden(const float* x, int64_t n_nodes, const float* hidden,
                           const float* hidden_absmax, int64_t n_edges,
                           const int32_t* rowptr, const int32_t* src, const int32_t* dst,
                           int n_layers, const int32_t* dims, const void* packed, const float* root,
                           const float* bias, int aggr, float* out, void* ws, size_t ws_bytes,
                           void* stream);
/* attributes: edge_attr + perm, or node_attr + src + dst (as gpde_hidden_fwd) */
GPDE_API int gpde_hidden_bwd(const float* edge_attr, const GpdeNodeAttr* node_attr, int64_t n_edges, const int32_t* perm,
                    const int32_t* src, const int32_t* dst, int n_layers,
                    const int32_t* dims, const float* const* W, const float* const* b,
                    const float* grad_hidden, float* const* grad_W, float* const* grad_b, void* ws,
                    size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Keep-Z pair (training): the forward already forms Z_i = sum_{e -> i} x_j (x) h_e for every node and the
 * backward's dW_3 = sum_i gT_i (x) Z_i needs exactly that; without it the backward re-aggregates it from
 * the recomputed (or given) hidden activations.  gpde_nnconv_fwd_keepz = gpde_nnconv_fwd (hidden == NULL) or
 * gpde_nnconv_fwd_hidden (hidden != NULL; edge_attr / perm unused) writing Z into z_keep [N][64][K2P] (K2P = last hidden
 * width padded to 128; ZERO-INITIALISED by the caller: nodes without in-edges are not written); the per-edge last layer of
 * low in-degree graphs is not taken.  The backward takes that buffer as `z_saved` (gpde_nnconv_bwd, gpde_nnconv_bwd_light). */
GPDE_API int gpde_nnconv_fwd_keepz(const float* x, int64_t n_nodes, const float* edge_attr, const float* hidden,
                          const float* hidden_absmax, int64_t n_edges, const int32_t* rowptr, const int32_t* src,
                          const int32_t* dst, const int32_t* perm, int n_layers, const int32_t* dims, const void* packed,
                          const float* root, const float* bias, int aggr, uint32_t flags, float* z_keep, float* out,
                          void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Depth-deferred backward (SURVEY.md §8 rows f1 x f4 when the hidden activations do NOT fit memory: H of the 241^2 graph is
 * 391 GB).  `KernelNN.forward` applies the SAME conv1 `depth` times (UAI1_full_resolution.py:29-30) and `loss.backward()`
 * (:266) sums the kernel MLP's gradients over those applications.  With dU_2^(l)[e] = (x_j^(l) . dZ_i^(l)) (.) [H_2[e] > 0]
 * and H_2 the same in every application, the sum over l can be taken BEFORE the hidden layers' backward:
 *   dU_2[e][k] = (sum_l sum_c x_j^(l)[c] dZ_i^(l)[c][k]) (.) [H_2[e][k] > 0]       one K = 64 * depth contraction per edge
 * so the two 1024 x 1024 GEMMs per edge (dU_1, dW_2), the transposes and dW_1 / db_* run ONCE per step.
 *   gpde_nnconv_bwd_light     one application: grad_x, grad of the last Linear (grad_w_last [4096][k2], grad_b_last [4096]),
 *                             grad_root, grad_bias - everything gpde_nnconv_bwd writes except the hidden layers'
 *                             gradients.  z_saved: NULL or the keep-Z forward's buffer (gpde_nnconv_fwd_keepz).
 *                             Workspace: gpde_nnconv_bwd_workspace_bytes.
 *   gpde_nnconv_bwd_deferred  all applications: x_stack [Lp][N][64] = the inputs x^(l) of the n_defer applications, ZERO
 *                             layers appended up to Lp = max(4, n_defer rounded up to even); grad_out_stack [n_defer][N][64] =
 *                             their output gradients (any order, the same in both stacks).  Writes grad_W[l] / grad_b[l] of
 *                             the hidden layers l = 0 .. n_layers - 2 (the last entries are ignored).  Workspace:
 *                             gpde_nnconv_bwd_deferred_workspace_bytes.
 * hidden_part / hidden_nodes (both entry points; NULL / 0: none): the last hidden activations of the in-edges of nodes
 * [0, hidden_nodes) as gpde_hidden_fwd(n_nodes = hidden_nodes) wrote them (the partial H of gpde_nnconv_fwd_mixed_keepz) - node
 * chunks below that bound read them instead of recomputing the hidden chain (the 241^2 graph: 44 % of the edges fit 170 GB).
 * Built for the kernel MLPs gpde_nnconv_bwd_deferred_supported() accepts (3 Linear layers, hidden widths multiples of 128,
 * at most 7 attributes: the split-f16 path); others return GPDE_EUNSUPPORTED - use gpde_nnconv_bwd per application.
 * Results: grad_x etc. of the light pass are the bits of gpde_nnconv_bwd (source-ordered); the hidden layers' gradients equal the
 * sum of the per-application ones up to fp32 / split-f16 summation order (tests/test_gpu_deferred.py: <= 2e-5). */
GPDE_API int gpde_nnconv_bwd_deferred_supported(int n_layers, const int32_t* dims);
GPDE_API size_t gpde_nnconv_bwd_deferred_workspace_bytes(int64_t n_nodes, int64_t n_edges, int n_layers, const int32_t* dims,
                                                int n_defer);
GPDE_API int gpde_nnconv_bwd_light(const float* x, int64_t n_nodes, const float* edge_attr, const GpdeNodeAttr* node_attr,
                          int64_t n_edges, const int32_t* rowptr,
                          const int32_t* src, const int32_t* dst, const int32_t* perm, const int32_t* rowptr_host,
                          const int32_t* src_rowptr, const int32_t* src_slots, int n_layers, const int32_t* dims,
                          const float* const* W, const float* const* b, const float* root, int aggr, const float* grad_out,
                          const float* z_saved, const float* hidden_part, int64_t hidden_nodes, float* grad_x,
                          float* grad_w_last, float* grad_b_last, float* grad_root,
                          float* grad_bias, void* ws, size_t ws_bytes, void* stream);
GPDE_API int gpde_nnconv_bwd_deferred(const float* x_stack, const float* grad_out_stack, int n_defer, int64_t n_nodes,
                             const float* edge_attr, const GpdeNodeAttr* node_attr, int64_t n_edges, const int32_t* rowptr,
                             const int32_t* src, const int32_t* dst, const int32_t* perm, const int32_t* rowptr_host,
                             int n_layers, const int32_t* dims, const float* const* W, const float* const* b, int aggr,
                             const float* hidden_part, int64_t hidden_nodes,
                             float* const* grad_W, float* const* grad_b, void* ws, size_t ws_bytes, void* stream);
/* The GENERAL forward.  Mixed call for graphs whose H does not fit memory (E * K2P * 4 bytes: 391 GB at the 241^2 graph):
 * `hidden` holds the rows of the in-edges of nodes [0, hidden_nodes) only (CSR slots [0, rowptr[hidden_nodes]); build it with
 * gpde_hidden_fwd(..., n_edges = rowptr[hidden_nodes], n_nodes = hidden_nodes)); those nodes aggregate from it, all others run the
 * fused kernel on the attributes.  Same result as gpde_nnconv_fwd.  3-Linear kernel MLPs. */
GPDE_API int gpde_nnconv_fwd_mixed_keepz(const float* x, int64_t n_nodes, const float* edge_attr, const GpdeNodeAttr* node_attr,
                                const float* hidden, const float* hidden_absmax, int64_t hidden_nodes, int64_t n_edges,
                                const int32_t* rowptr, const int32_t* src, const int32_t* dst,
                                const int32_t* perm, int n_layers, const int32_t* dims, const void* packed,
                                const float* root, const float* bias, int aggr, uint32_t flags, float* z_keep, float* out,
                                void* ws, size_t ws_bytes, void* stream);
/* ^ attributes from edge_attr + perm or from node_attr (then edge_attr / perm may be NULL); hidden_nodes = 0 / hidden = NULL: no
 *   partial H; z_keep (as in gpde_nnconv_fwd_keepz) = NULL: Z not kept.  (Round 5 folded the mixed, node-table and node-table +
 *   partial-H forwards of round 4 into this call.) */

/* ---------------------------------------------------------------------------------------------
 * The operator given the PER-EDGE WEIGHTS (second half; row a6 'max').
 * `weight = self.nn(pseudo).view(-1, in, out)` (nn_conv.py:274) is what the reference forms on every call.  For the
 * MGKN V-cycles' low in-degree / small graphs (MGKN_orthogonal_burgers1d.py:73-82: 2-3 in-edges per node;
 * MGKN_general_darcy2d.py:76-90: coarse levels of a few thousand edges) the same module runs `depth` times per forward
 * with the same edge_attr and weights, so that tensor is the same in every call: gpde_edge_weights_fwd builds it once
 * from the hidden activations of gpde_hidden_fwd ([E][4096] fp32 in CSR slot order, the last Linear's bias folded in),
 * and gpde_nnconv_fwd_edgeweights_group then runs any number of INDEPENDENT calls in one launch each doing gather,
 * message (nn_conv.py:275), aggregation (add / mean / max) and update() (nn_conv.py:277-282; + opt-in residual and
 * ReLU, the callers' `relu(x + conv(x))` glue) in a single streaming kernel (forward; its backward pair follows below). */
GPDE_API size_t gpde_edge_weights_workspace_bytes(int64_t n_edges, int n_layers, const int32_t* dims);
GPDE_API int gpde_edge_weights_fwd(const float* hidden /* [E][K2P], gpde_hidden_fwd */, int64_t n_edges, int n_layers,
                          const int32_t* dims, const void* packed /* gpde_mlp_pack image (k2 padded >= 256), else unused */,
                          const float* w_last /* [4096][k2] */, const float* b_last /* [4096] or NULL */,
                          float* edge_weights /* [E][4096] */, void* ws, size_t ws_bytes, void* stream);
#define GPDE_WECONV_MAX_GROUP 16 /* descriptors per launch; longer lists take several launches */
typedef struct GpdeWeConvDesc {
    const float* x;            /* [n_nodes][64] */
    const float* edge_weights; /* [E][4096] from gpde_edge_weights_fwd, CSR slot order */
    const int32_t* rowptr;     /* [n_nodes + 1] destination CSR (gpde_csr_from_coo) */
    const int32_t* src;        /* [E] source node per CSR slot */
    const float* root;         /* [64][64] or NULL */
    const float* bias;         /* [64] or NULL */
    const float* residual;     /* [n_nodes][64] or NULL: out = act(residual + NNConv(x)) */
    float* out;                /* [n_nodes][64] */
    int32_t n_nodes;
    int32_t aggr;              /* GPDE_AGGR_ADD | GPDE_AGGR_MEAN | GPDE_AGGR_MAX */
    int32_t relu;              /* 1: ReLU on the result */
    int32_t reserved;
} GpdeWeConvDesc;
GPDE_API int gpde_nnconv_fwd_edgeweights_group(const GpdeWeConvDesc* descs /* HOST array */, int n_descs, void* stream);

/* Training on the per-edge weights (both MGKN scripts are training scripts: MGKN_general_darcy2d.py:260-282,
 * MGKN_orthogonal_burgers1d.py:226-242).  W_e is an autograd node shared by the `depth` applications of a module:
 *   gpde_nnconv_bwd_edgeweights  backward of the operator given W_e: grad_x [N][64] (ordered over each source's out-edges
 *                                when src_rowptr / src_slots are given, else fp32 atomics), grad_edge_weights [E][4096]
 *                                = x_j (x) gT_i (what autograd forms for `weight` in nn_conv.py:274-275), grad_root,
 *                                grad_bias (NULL to skip).  'add' / 'mean'.
 *   gpde_edge_weights_bwd        backward of gpde_edge_weights_fwd given the SUM of grad_edge_weights over the applications:
 *                                grad_hidden [E][K2P] = (grad_W_e . W3) (.) [hidden > 0] (the input of gpde_hidden_bwd),
 *                                grad_w_last [4096][k2], grad_b_last [4096] - the two 4096 x k2 products per edge once per
 *                                step instead of once per application, on the split-f16 GEMMs. */
GPDE_API size_t gpde_nnconv_bwd_edgeweights_workspace_bytes(int64_t n_nodes, int64_t n_edges);
GPDE_API int gpde_nnconv_bwd_edgeweights(const float* x, int64_t n_nodes, const float* edge_weights, int64_t n_edges,
                                const int32_t* rowptr, const int32_t* src, const int32_t* src_rowptr,
                                const int32_t* src_slots, const float* root, int aggr, const float* grad_out,
                                float* grad_x, float* grad_edge_weights, float* grad_root, float* grad_bias, void* ws,
                                size_t ws_bytes, void* stream);
/* ... the same call adding into gradients that already hold the sum of the module's earlier applications of this backward pass
 * (`accumulate`: GPDE_ACC_* bits; 0 = gpde_nnconv_bwd_edgeweights).  What autograd's `grad = grad + new` does for a tensor used
 * by several applications (the reference's MGKN loops apply each NNConv `depth` times, MGKN_general_darcy2d.py:76-90): one
 * elementwise kernel per application and gradient - 16 KiB per edge read twice and written once for W_e.  In-kernel: the same
 * additions in the same order (unfused multiply, then add: the same bits), the old value read once. */
enum {
    GPDE_ACC_EDGE_WEIGHTS = 1,   /* grad_edge_weights[e] += x_j (x) gT_i */
    GPDE_ACC_ROOT = 2,           /* grad_root += X^T g */
    GPDE_ACC_BIAS = 4            /* grad_bias += colsum g */
};
GPDE_API int gpde_nnconv_bwd_edgeweights_acc(const float* x, int64_t n_nodes, const float* edge_weights, int64_t n_edges,
                                    const int32_t* rowptr, const int32_t* src, const int32_t* src_rowptr,
                                    const int32_t* src_slots, const float* root, int aggr, const float* grad_out,
                                    float* grad_x, float* grad_edge_weights, float* grad_root, float* grad_bias,
                                    int accumulate, void* ws, size_t ws_bytes, void* stream);
GPDE_API size_t gpde_edge_weights_bwd_workspace_bytes(int64_t n_edges, int n_layers, const int32_t* dims);
GPDE_API int gpde_edge_weights_bwd(const float* grad_edge_weights, const float* hidden, int64_t n_edges, int n_layers,
                          const int32_t* dims, const float* w_last, float* grad_hidden, float* grad_w_last,
                          float* grad_b_last, void* ws, size_t ws_bytes, void* stream);

/* The operator given the per-edge weights at ANY width (gpde_weconv_any.hip): the reference's classes take any in_channels and
 * out_channels (nn_conv.py:234-241; the message is `nn(pseudo).view(-1, in_channels, out_channels)`, nn_conv.py:274), the calls
 * above are built for 64 -> 64.  Same mathematics, run-time widths 1 <= in_channels, out_channels <= GPDE_WECONV_ANY_MAX_WIDTH:
 *   x [N][in], edge_weights [E][in * out] (row-major [in][out] per edge, rows in CSR slot order), root [in][out] or NULL,
 *   bias [out] or NULL, residual [N][out] or NULL (must not alias out), out [N][out]; aggr add / mean / max in the forward
 *   (mean divides by clamp(count, 1); a node without in-edges aggregates to 0, also for max), add / mean in the backward
 *   (GPDE_AGGR_MAX: GPDE_EUNSUPPORTED - its gradient is composed by the caller).
 *   Backward outputs grad_x [N][in], grad_edge_weights [E][in * out] (required when n_edges > 0), grad_root [in][out],
 *   grad_bias [out]; NULL skips grad_x / grad_root / grad_bias.  grad_x is summed over each source's out-edges in ascending slot
 *   order when src_rowptr / src_slots (gpde_csr_source_order) are given, else by fp32 atomics.
 * Plain fp32 fmaf in a summation order fixed by the shapes: two calls give the same bits.  Widths outside the range:
 * GPDE_EUNSUPPORTED; zero nodes / zero edges are valid calls.  These entry points are additions: GPDE_VERSION is unchanged, and
 * a binding generated from this header fails to load a library that lacks them (it resolves every declared symbol). */
#define GPDE_WECONV_ANY_MAX_WIDTH 256
GPDE_API int gpde_nnconv_fwd_edgeweights_any(const float* x, int64_t n_nodes, const float* edge_weights, int64_t n_edges,
                                    const int32_t* rowptr, const int32_t* src, const float* root, const float* bias,
                                    const float* residual, int relu, int aggr, int in_channels, int out_channels,
                                    float* out, void* stream);
GPDE_API size_t gpde_nnconv_bwd_edgeweights_any_workspace_bytes(int64_t n_nodes, int64_t n_edges, int in_channels,
                                                       int out_channels);
/* Host only: the lane tiling gpde_weconv_any.hip runs at these widths - out[0..5] = V (floats per column access: 4 or 1),
 * LC (column lanes), R (row lanes), ES (edge slots per wave), B (x_j batches gathered into LDS per pass; a pass is B * ES
 * in-edges), LC * R * ES (lanes of the 64 in use) - from the function the two launchers call.  vec4 != 0: out_channels % 4 == 0 and
 * every buffer 16-byte aligned (what the launchers test; at out_channels % 4 != 0 the answer is the V = 1 tiling either way);
 * aggr GPDE_AGGR_MAX: the forward's tiling for 'max' (R = 1).  GPDE_EUNSUPPORTED outside the widths, GPDE_EINVAL for a NULL out or
 * an unknown aggr. */
GPDE_API int gpde_nnconv_edgeweights_any_plan(int in_channels, int out_channels, int vec4, int aggr, int32_t* out);
GPDE_API int gpde_nnconv_bwd_edgeweights_any(const float* x, int64_t n_nodes, const float* edge_weights, int64_t n_edges,
                                    const int32_t* rowptr, const int32_t* src, const int32_t* src_rowptr,
                                    const int32_t* src_slots, const float* root, int aggr, int in_channels,
                                    int out_channels, const float* grad_out, float* grad_x, float* grad_edge_weights,
                                    float* grad_root, float* grad_bias, void* ws, size_t ws_bytes, void* stream);

/* The RE-ASSOCIATED operator at any width (gpde_reassoc_any.hip): for a Linear / ReLU chain `nn` and aggr add / mean the last
 * Linear commutes with the aggregation, so [E][in * out] need not be formed (what the 64-wide entry points have always done,
 * DESIGN.md §2).  The caller gives the LAST HIDDEN ACTIVATIONS instead of the per-edge weights:
 *   x [N][in], hidden [E][k_hidden] = relu(L_{n-1}(... pseudo)) with rows in CSR slot order (no padding), w_last [in * out][k_hidden]
 *   and b_last [in * out] (nullable) in torch's layouts, root [in][out] or NULL, bias [out] or NULL, out [N][out]:
 *     Z'_d = [sum_{e -> d} x_src(e) (x) hidden_e | sum_{e -> d} x_src(e)]        per destination node, [in][k_hidden + 1]
 *     out_d = Z'_d . [W_last | b_last] (/ clamp(count_d, 1) for mean) + x_d . root + bias
 *   1 <= in_channels, out_channels <= GPDE_WECONV_ANY_MAX_WIDTH, 1 <= k_hidden <= GPDE_REASSOC_ANY_MAX_HIDDEN; anything else and
 *   GPDE_AGGR_MAX (not linear in the last Linear): GPDE_EUNSUPPORTED.  Zero nodes / zero edges are valid calls.
 *   Backward outputs (overwritten): grad_x [N][in], grad_hidden [E][k_hidden] = dL/d hidden (NOT masked by hidden > 0: the
 *   caller's autograd differentiates its own ReLU; required when n_edges > 0), grad_w_last [in * out][k_hidden], grad_b_last
 *   [in * out], grad_root [in][out], grad_bias [out]; NULL skips any of the others.  grad_x is summed over each source's out-edges
 *   in ascending slot order: src_rowptr / src_slots (gpde_csr_source_order) are required with grad_x when n_edges > 0.
 * Workspace: Z' is in * (k_hidden + 1) * 4 bytes per node (1 MiB at 256 x 1024), so both calls walk blocks of destination nodes
 * sized to the workspace they are given.  *_workspace_bytes returns the preferred size; a smaller workspace gives more blocks of
 * fewer nodes, down to one node; less than one node's worth: GPDE_EINVAL (the message names the size).  Calls without edges use no
 * node block: the forward and a zero-node backward take ws = NULL, a zero-edge backward needs a workspace only for grad_root /
 * grad_bias (their strip partials; any size the query returns is enough).
 * Plain fp32 (fmaf; fp32 MFMA in the node-side GEMMs), no atomics, in-edges in ascending slot order, long rows summed two-level
 * (DESIGN.md §3).  The summation order is fixed by the shapes and the workspace size: two identical calls give identical bits,
 * and out / grad_x / grad_hidden do not depend on the number of node blocks (grad_w_last / grad_b_last are summed over the
 * blocks in order).  Additions to the ABI like the block above: GPDE_VERSION is unchanged. */
#define GPDE_REASSOC_ANY_MAX_HIDDEN 4096
GPDE_API size_t gpde_nnconv_fwd_hidden_any_workspace_bytes(int64_t n_nodes, int64_t n_edges, int in_channels, int out_channels,
                                                  int k_hidden);
GPDE_API int gpde_nnconv_fwd_hidden_any(const float* x, int64_t n_nodes, const float* hidden, int64_t n_edges, int k_hidden,
                               const int32_t* rowptr, const int32_t* src, const float* w_last, const float* b_last,
                               const float* root, const float* bias, int aggr, int in_channels, int out_channels, float* out,
                               void* ws, size_t ws_bytes, void* stream);
GPDE_API size_t gpde_nnconv_bwd_hidden_any_workspace_bytes(int64_t n_nodes, int64_t n_edges, int in_channels, int out_channels,
                                                  int k_hidden);
GPDE_API int gpde_nnconv_bwd_hidden_any(const float* x, int64_t n_nodes, const float* hidden, int64_t n_edges, int k_hidden,
                               const int32_t* rowptr, const int32_t* src, const float* w_last, const float* b_last,
                               const float* root, int aggr, int in_channels, int out_channels, const float* grad_out,
                               float* grad_x, float* grad_hidden, float* grad_w_last, float* grad_b_last, float* grad_root,
                               float* grad_bias, const int32_t* src_rowptr, const int32_t* src_slots, void* ws, size_t ws_bytes,
                               void* stream);

/* The two any-width operators BETWEEN TWO NODE SETS (bipartite graphs; torch_geometric.nn.NNConv's `x = (x_src, x_dst)`,
 * `size = (n_src, n_dst)`, `in_channels = (in_src, in_dst)`): evaluation of the kernel integral at query points, restriction /
 * prolongation between the levels of a V-cycle.  Edges (j in [0, n_src)) -> (i in [0, n_dst)), the CSR of gpde_csr_from_coo2:
 *     out_i = aggr_{e: j -> i} x_src[j] . W_e  (+ x_dst[i] . root when x_dst and root are given)  + bias        out [n_dst][out]
 *   x_src [n_src][in_src], x_dst [n_dst][in_dst] or NULL (PyG: `x_r = x[1]; if x_r is not None and root_weight: out += lin(x_r)`),
 *   W_e [in_src][out] per edge, root [in_dst][out] or NULL, residual [n_dst][out] or NULL.  The arguments are those of the `_any`
 *   entry points above with the node table split in two; the SAME kernels run (the square entry points hand x_dst = x, in_dst =
 *   in_src, n_src = n_dst to them), so a rectangular call on a graph that happens to be square gives the square call's bits.
 *   Backward outputs: grad_x_src [n_src][in_src] - the sum over each source's out-edges, ascending slot order when src_rowptr /
 *   src_slots OVER n_src (gpde_csr_source_order(src, n_edges, n_src, ...)) are given, else fp32 atomics (edge-weight form; the
 *   hidden form requires them with grad_x_src when n_edges > 0); it has NO root term - grad_x_dst [n_dst][in_dst] = g . root^T
 *   (zero without root), grad_root [in_dst][out] = x_dst^T g, grad_bias = colsum g; the others as in `_any`.  Any of grad_x_src /
 *   grad_x_dst / grad_root / grad_bias may be NULL.
 *   Errors: root, grad_root or grad_x_dst != NULL with x_dst == NULL and n_dst > 0: GPDE_EINVAL; in_dst outside 1 .. GPDE_WECONV_ANY_MAX_WIDTH
 *   (also when x_dst == NULL: pass in_src): GPDE_EUNSUPPORTED; GPDE_AGGR_MAX in a backward (and in the hidden form): GPDE_EUNSUPPORTED.
 *   n_src == 0, n_dst == 0 and n_edges == 0 are valid calls (edges need both sets non-empty: GPDE_EINVAL otherwise).
 *   Workspaces: the *_bip_workspace_bytes queries (the forward of the hidden form depends on n_dst and in_src only); the node
 *   blocks of the hidden form walk the n_dst destinations, Z' is [in_src][k_hidden + 1] per destination.
 * The same documented properties: plain fp32 fmaf, two-level sums, no atomics except an un-ordered grad_x_src, a summation order
 * fixed by the shapes.  Additions to the ABI: GPDE_VERSION is unchanged. */
GPDE_API int gpde_nnconv_fwd_edgeweights_bip(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst,
                                    const float* edge_weights, int64_t n_edges, const int32_t* rowptr, const int32_t* src,
                                    const float* root, const float* bias, const float* residual, int relu, int aggr,
                                    int in_src, int in_dst, int out_channels, float* out, void* stream);
GPDE_API size_t gpde_nnconv_bwd_edgeweights_bip_workspace_bytes(int64_t n_src, int64_t n_dst, int64_t n_edges, int in_src,
                                                       int in_dst, int out_channels);
GPDE_API int gpde_nnconv_bwd_edgeweights_bip(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst,
                                    const float* edge_weights, int64_t n_edges, const int32_t* rowptr, const int32_t* src,
                                    const int32_t* src_rowptr, const int32_t* src_slots, const float* root, int aggr,
                                    int in_src, int in_dst, int out_channels, const float* grad_out, float* grad_x_src,
                                    float* grad_x_dst, float* grad_edge_weights, float* grad_root, float* grad_bias,
                                    void* ws, size_t ws_bytes, void* stream);
GPDE_API size_t gpde_nnconv_fwd_hidden_bip_workspace_bytes(int64_t n_dst, int64_t n_edges, int in_src, int out_channels,
                                                  int k_hidden);
GPDE_API int gpde_nnconv_fwd_hidden_bip(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst,
                               const float* hidden, int64_t n_edges, int k_hidden, const int32_t* rowptr,
                               const int32_t* src, const float* w_last, const float* b_last, const float* root,
                               const float* bias, int aggr, int in_src, int in_dst, int out_channels, float* out,
                               void* ws, size_t ws_bytes, void* stream);
GPDE_API size_t gpde_nnconv_bwd_hidden_bip_workspace_bytes(int64_t n_dst, int64_t n_edges, int in_src, int in_dst,
                                                  int out_channels, int k_hidden);
GPDE_API int gpde_nnconv_bwd_hidden_bip(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst,
                               const float* hidden, int64_t n_edges, int k_hidden, const int32_t* rowptr,
                               const int32_t* src, const float* w_last, const float* b_last, const float* root, int aggr,
                               int in_src, int in_dst, int out_channels, const float* grad_out, float* grad_x_src,
                               float* grad_x_dst, float* grad_hidden, float* grad_w_last, float* grad_b_last,
                               float* grad_root, float* grad_bias, const int32_t* src_rowptr, const int32_t* src_slots,
                               void* ws, size_t ws_bytes, void* stream);

/* The re-associated any-width operator FROM THE EDGE ATTRIBUTES (gpde_chain_any.hip): the operator of the "hidden form" above with
 * `hidden` replaced by its definition for a Linear / ReLU chain of n_linear = 2 .. 5 Linears,
 *     hidden = relu(L_{n-1}(... relu(L_1(edge_attr)) ...)),     dims = [k0, K_1, .., K_{n-1}, in_src * out]     (n_linear + 1 entries)
 *   1 <= k0 <= 64, 1 <= K_l <= GPDE_REASSOC_ANY_MAX_HIDDEN, widths and aggr as the hidden form (add / mean).  The hidden rows are
 *   generated BY BLOCK OF CONSECUTIVE DESTINATIONS and never exist for more than one block: no caller-side tensor is [E][K] or
 *   [E][in * out].  One entry point serves one node set (`square` != 0: x_src is the table of the root term too, x_dst / n_src /
 *   in_dst / grad_x_dst are ignored, grad_x_src holds both terms in one ordered sum) and two (`square` == 0: the `_bip` rules).
 *   edge_attr [E][k0] and grad_edge_attr [E][k0]: rows in CSR SLOT order (the convention `hidden` has above).
 *   weights / biases: HOST arrays of n_linear device pointers in torch's layouts (W_l [K_l][K_{l-1}], b_l [K_l]; `biases` or any
 *   entry of it may be NULL: no bias); grad_w / grad_b likewise (the array or any entry NULL: that gradient is not formed).
 * The block table.  The hidden rows of the block of destinations [a, b) are the CSR slots rowptr[a] .. rowptr[b]; the host must know
 *   that count to size buffers and grids and the library never synchronises, so the table is a HOST argument: block_nodes holds
 *   n_blocks + 1 pairs (first node, first slot) - pair b opens block b, the last pair is (n_dst, n_edges).
 *   gpde_nnconv_chain_any_plan   HOST ONLY, no device call.  From a host copy of rowptr: cuts consecutive destinations greedily so
 *     that a block's per-edge buffers of the BACKWARD stay within budget_bytes.  A block is never less than one node - a row larger
 *     than the budget is a block of its own and the sizes returned cover it -, nodes without in-edges join their neighbour's block.
 *     block_nodes_out: room for 2 * (n_dst + 1) int32, or NULL (count and sizes only).  A block of 2^31 or more elements
 *     (rows x widest K_l): GPDE_EUNSUPPORTED.  *ws_fwd / *ws_bwd: the workspaces the two calls need WITH THIS TABLE.
 *   gpde_nnconv_chain_any_workspace_bytes   HOST ONLY: the same two sizes for a table the caller made.
 *   A table that is not monotone, does not run from (0, 0) to (n_dst, n_edges) or has slots in a block without nodes: GPDE_EINVAL.
 *   A workspace below the size the table needs: GPDE_EWORKSPACE (the message names the size).  A table whose slots disagree with the
 *   device rowptr cannot be seen from the host: the kernels then read a copy of rowptr clipped to each block's slot range, so they
 *   stay inside the block's buffers (the results are wrong), and *n_bad (int32 device word, nullable; cleared by the call) is set.
 * Memory.  The workspace holds, besides the last Linear permuted (and its gradient), the buffers of ONE block: in the forward two
 *   [E_b][max K_l] buffers; in the backward every layer's activations, dH and two dU buffers - gpde_nnconv_chain_any_plan's budget -
 *   and Z' (dZ') of a node sub-block of at most that many bytes.  What remains O(E): the caller's edge_attr (and grad_edge_attr) and,
 *   in the backward's workspace, the per-edge dx rows [E][in_src] of the ordered grad_x_src sum.
 * Determinism.  fp32, no atomics.  out, grad_x_src, grad_x_dst and grad_edge_attr do not depend on the block table, bit for bit (a
 *   hidden row's arithmetic does not depend on its block); the weight and bias gradients are summed over the blocks in order.  The
 *   derivative of the ReLU at 0 is 0, as torch's.  A NULL gradient output leaves the bits of the others unchanged.
 * Zero destinations and zero edges are valid calls.  Additions to the ABI: GPDE_VERSION is unchanged. */
GPDE_API int gpde_nnconv_chain_any_plan(const int32_t* rowptr_host, int64_t n_dst, int64_t n_edges, int n_linear, const int32_t* dims,
                               int in_src, int in_dst, int out_channels, size_t budget_bytes, int32_t* block_nodes_out,
                               int64_t* n_blocks, size_t* ws_fwd, size_t* ws_bwd);
GPDE_API int gpde_nnconv_chain_any_workspace_bytes(const int32_t* block_nodes, int64_t n_blocks, int64_t n_dst, int64_t n_edges,
                                          int n_linear, const int32_t* dims, int in_src, int in_dst, int out_channels,
                                          size_t* ws_fwd, size_t* ws_bwd);
GPDE_API int gpde_nnconv_fwd_chain_any(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst, int square,
                              const float* edge_attr, int64_t n_edges, const int32_t* rowptr, const int32_t* src, int n_linear,
                              const int32_t* dims, const float* const* weights, const float* const* biases, const float* root,
                              const float* bias, int aggr, int in_src, int in_dst, int out_channels, const int32_t* block_nodes,
                              int64_t n_blocks, float* out, int32_t* n_bad, void* ws, size_t ws_bytes, void* stream);
GPDE_API int gpde_nnconv_bwd_chain_any(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst, int square,
                              const float* edge_attr, int64_t n_edges, const int32_t* rowptr, const int32_t* src, int n_linear,
                              const int32_t* dims, const float* const* weights, const float* const* biases, const float* root,
                              int aggr, int in_src, int in_dst, int out_channels, const float* grad_out, float* grad_x_src,
                              float* grad_x_dst, float* grad_edge_attr, float* const* grad_w, float* const* grad_b, float* grad_root,
                              float* grad_bias, const int32_t* src_rowptr, const int32_t* src_slots, const int32_t* block_nodes,
                              int64_t n_blocks, int32_t* n_bad, void* ws, size_t ws_bytes, void* stream);

/* The same operator for a chain whose hidden layers have OTHER ACTIVATIONS than the ReLU (gpde_chain_any.hip):
 *     hidden = act_{n-1}(L_{n-1}(... act_1(L_1(edge_attr)) ...)),     one kind per hidden layer, mixed chains allowed.
 *   The four entry points below mirror the `_chain_any` four argument for argument, with two more HOST arrays after `dims`:
 *     act_kinds   n_linear - 1 entries, GPDE_ACT_* (NULL: all GPDE_ACT_RELU);
 *     act_params  [n_linear - 1][2] floats (NULL: zeros): [l][0] is LEAKY_RELU's slope (finite, >= 0) or ELU's alpha (finite, > 0),
 *                 [l][1] is reserved (finite).
 *   An unknown kind: GPDE_EUNSUPPORTED; a slope < 0, an alpha <= 0 or a non-finite parameter: GPDE_EINVAL.  A table and its workspace
 *   sizes belong to the kinds they were asked for.  The `_chain_any` entry points are the all-RELU call of the same body; an all-RELU
 *   call here gives their sizes and their bits.
 *     kind                   h = act(u)                                act' is computed from
 *     GPDE_ACT_RELU          max(u, 0)                                 h   (h > 0)
 *     GPDE_ACT_LEAKY_RELU    u > 0 ? u : slope u                       h   (h > 0 ? 1 : slope)
 *     GPDE_ACT_ELU           u > 0 ? u : alpha (e^u - 1)               h   (h > 0 ? 1 : h + alpha)
 *     GPDE_ACT_TANH          tanh u                                    h   (1 - h^2)
 *     GPDE_ACT_SIGMOID       1 / (1 + e^-u)                            h   (h (1 - h))
 *     GPDE_ACT_GELU          u (1 + erf(u / sqrt 2)) / 2               u
 *     GPDE_ACT_GELU_TANH     torch's GELU(approximate='tanh')          u
 *     GPDE_ACT_SILU          u / (1 + e^-u)                            u
 *     GPDE_ACT_SIN           sin u                                     u
 *   fp32 with the accurate device functions; branches select, so a saturated unit (|u| past expf's range) gives its finite limit.
 *   Memory: a kind whose derivative comes from h keeps what the ReLU chain keeps; one that needs u keeps U_l next to H_l in the
 *   backward's recompute pass - one more [block edges][K_l padded to 4] buffer per such layer, counted by the plan's budget (fewer
 *   edges per block) and by *ws_bwd.  *ws_fwd does not depend on the kinds.  Determinism as above, for every kind.
 * Additions to the ABI: GPDE_VERSION is unchanged. */
#define GPDE_ACT_RELU 0
#define GPDE_ACT_LEAKY_RELU 1
#define GPDE_ACT_ELU 2
#define GPDE_ACT_TANH 3
#define GPDE_ACT_SIGMOID 4
#define GPDE_ACT_GELU 5
#define GPDE_ACT_GELU_TANH 6
#define GPDE_ACT_SILU 7
#define GPDE_ACT_SIN 8
GPDE_API int gpde_nnconv_chain_act_plan(const int32_t* rowptr_host, int64_t n_dst, int64_t n_edges, int n_linear, const int32_t* dims,
                               const int32_t* act_kinds, const float* act_params, int in_src, int in_dst, int out_channels,
                               size_t budget_bytes, int32_t* block_nodes_out, int64_t* n_blocks, size_t* ws_fwd, size_t* ws_bwd);
GPDE_API int gpde_nnconv_chain_act_workspace_bytes(const int32_t* block_nodes, int64_t n_blocks, int64_t n_dst, int64_t n_edges,
                                          int n_linear, const int32_t* dims, const int32_t* act_kinds, const float* act_params,
                                          int in_src, int in_dst, int out_channels, size_t* ws_fwd, size_t* ws_bwd);
GPDE_API int gpde_nnconv_fwd_chain_act(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst, int square,
                              const float* edge_attr, int64_t n_edges, const int32_t* rowptr, const int32_t* src, int n_linear,
                              const int32_t* dims, const int32_t* act_kinds, const float* act_params, const float* const* weights,
                              const float* const* biases, const float* root, const float* bias, int aggr, int in_src, int in_dst,
                              int out_channels, const int32_t* block_nodes, int64_t n_blocks, float* out, int32_t* n_bad, void* ws,
                              size_t ws_bytes, void* stream);
GPDE_API int gpde_nnconv_bwd_chain_act(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst, int square,
                              const float* edge_attr, int64_t n_edges, const int32_t* rowptr, const int32_t* src, int n_linear,
                              const int32_t* dims, const int32_t* act_kinds, const float* act_params, const float* const* weights,
                              const float* const* biases, const float* root, int aggr, int in_src, int in_dst, int out_channels,
                              const float* grad_out, float* grad_x_src, float* grad_x_dst, float* grad_edge_attr,
                              float* const* grad_w, float* const* grad_b, float* grad_root, float* grad_bias,
                              const int32_t* src_rowptr, const int32_t* src_slots, const int32_t* block_nodes, int64_t n_blocks,
                              int32_t* n_bad, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Edge attributes on the fly (opt-in): the `node_attr` argument (GpdeNodeAttr, declared at the top).
 * The reference materialises edge_attr[e] = [pos_src(2), pos_dst(2), a_src, a_dst] from node data
 * (SquareMeshGenerator.attributes, utilities.py:274-277; multi_pole_grid1d, multipole utilities.py:1771-1777): 24 of the 40
 * algorithmic bytes per edge and a 2.3 GB tensor on the 241^2 graph.  With node_attr the kernels read them from a node table
 * instead: slot d of edge (j -> i) is
 *     table[(sel[d] >> 8 ? i : j) * stride + (sel[d] & 255)]        (endpoint 0 = source j, 1 = target i)
 * Same result as the call on the materialised tensor (bitwise: the attribute values are the same floats;
 * tests/test_gpu_nodeattr.py, test_gpu_nodeattr_train.py).  Taken by the general forward, gpde_hidden_fwd, gpde_nnconv_bwd,
 * gpde_nnconv_bwd_light, gpde_nnconv_bwd_deferred and gpde_hidden_bwd - a training step on a graph built from positions
 * (gpde_radius_csr_*) needs neither the [E][k0] tensor nor its slot-order copy.  Built for 3-Linear kernel MLPs of >= 8 k1
 * chunks on the default GPDE_FWD_F16SPLIT kernels, 1..7 slots; anything else returns GPDE_EUNSUPPORTED / GPDE_EINVAL. */

/* ---------------------------------------------------------------------------------------------
 * Radius graph on the GPU.  Replaces SquareMeshGenerator / RandomMeshGenerator.ball_connectivity
 * (utilities.py:250-255, 362-368: dense float64 pairwise_distances + np.where).  pos_src / pos_dst [n][dim]
 * float64 (dim 1..3).  Pass 1 writes the out-degree of every source; the caller forms the
 * exclusive prefix sum `offsets` [n+1] (int64) and allocates edge_index int64 [2][E], E =
 * offsets[n]; pass 2 fills it: edges (j in pos_src -> i in pos_dst) within distance r, self-loops included, sorted by
 * source then target (row-major np.where) - the reference's order.  Two point sets, because that is what
 * the inner (pos_dst == pos_src) and inter-level graphs of RandomMultiMeshGenerator.ball_connectivity are
 * (multipole-graph-neural-operator/utilities.py:602-640: pairwise_distances(X, Y) <= r).  The choice of
 * arithmetic: flags = 0 tests sum_k (dx_k)^2 <= r^2 exactly in float64 (symmetric graphs);
 * GPDE_RADIUS_REFERENCE_TIES evaluates scikit-learn's dot-product expansion operation by operation, so that pairs at
 * exactly distance r are kept or dropped as in the reference (its default s = 61, r = 0.10 graph: 376,471 edges).
 * pos_dst == pos_src with n_dst == n_src means ONE point set: self-loops, diagonal forced to distance 0. */
enum { GPDE_RADIUS_REFERENCE_TIES = 1 };
GPDE_API int gpde_radius_graph2_count(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                             double r, uint32_t flags, int32_t* deg, void* stream);
GPDE_API int gpde_radius_graph2_fill(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                            double r, uint32_t flags, const int64_t* offsets, int64_t* edge_index, int64_t n_edges,
                            void* stream);

/* The same graphs by CELL LIST, emitted directly as the destination-sorted CSR the operator consumes (no int64 COO list,
 * no sort by destination; O(N * neighbourhood) tests instead of O(N^2)): the source points are binned into cells of
 * edge >= r, one wave per destination point walks the 3^dim neighbouring cells.  Pass 1 (count) builds the cell
 * structure in `ws` and writes the in-degree of every destination; the caller forms rowptr = exclusive scan (int32
 * [n_dst + 1]) and allocates src / dst int32 [E]; pass 2 (fill, same arguments, same untouched `ws`) writes them, each
 * row in ascending source order - exactly what gpde_csr_from_coo makes of the reference's source-major edge list
 * (rows longer than 4096 edges keep cell order).  lo / hi: HOST arrays [dim], a bounding box of both point sets.
 * Edge attributes for such a graph are addressed by CSR slot (perm = identity). */
GPDE_API size_t gpde_radius_csr_workspace_bytes(int64_t n_src, int dim, double r, const double* lo, const double* hi);
GPDE_API int gpde_radius_csr_count(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim, double r,
                          uint32_t flags, const double* lo, const double* hi, int32_t* deg, void* ws, size_t ws_bytes,
                          void* stream);
GPDE_API int gpde_radius_csr_fill(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim, double r,
                         uint32_t flags, const double* lo, const double* hi, const int32_t* rowptr, int32_t* src,
                         int32_t* dst, int64_t n_edges, void* ws, size_t ws_bytes, void* stream);

/* The cell-list builder on a PERIODIC box (torus), with the minimum-image edge geometry.  The reference's periodic problems
 * (Burgers with is_periodic=True, MGKN_orthogonal_burgers1d.py:165; RandomMeshGenerator.torus1d_connectivity, multipole
 * utilities.py:404-417; TorusGridSplitter.torus_connectivity / get_data, utilities.py:1190-1266) join points across the seam
 * and give the kernel network the WRAPPED displacement [dx, dy, |d|, a_i, a_j] - which endpoint coordinates cannot reproduce.
 * The arguments of the open twins plus
 *   origin[dim], period[dim]  HOST arrays: period[k] > 0 - axis k wraps with that length, measured from origin[k];
 *                             period[k] == 0 - an open axis, as in gpde_radius_csr_* (lo / hi are read on open axes only and
 *                             may be NULL when every axis is periodic);
 *   geom (fill, nullable)     float32 [E][dim + 1] by CSR slot: pos_src[j] - image(pos_dst[i]) per axis (source minus target, the
 *                             sign of the reference's X_difference with rows indexed by edge_index[0]; the plain difference on
 *                             open axes), then its Euclidean norm - float64 arithmetic, rounded to float32 once.
 * Points outside [origin, origin + period) are legal: they are reduced into it (x - L floor((x - o) / L), float64).  The test is
 * the exact float64 sum of squares of the minimum-image differences against r^2 (flags = 0; GPDE_RADIUS_REFERENCE_TIES has no
 * periodic form: the reference's torus code aliases its shifted grids and never wraps, so there is no tie behaviour to
 * reproduce).  2 r < period[k] is required on every periodic axis: each (source, destination) pair then has one nearest image
 * and gives at most one edge.  Rows as in the open builder: ascending source id (rows longer than 4096 edges keep cell order);
 * self-loops included.  Two passes with the caller's scan between them, `ws` untouched in between, like the open twins.
 * GPDE_EINVAL (before any device call) for dim outside 1..3, a negative period, 2 r >= period[k], r <= 0 and
 * GPDE_RADIUS_REFERENCE_TIES; the workspace query returns 0 for the ones it can see (gpde_last_error() names the argument).
 * Additions to the ABI: GPDE_VERSION is unchanged. */
GPDE_API size_t gpde_radius_csr_periodic_workspace_bytes(int64_t n_src, int dim, double r, const double* lo, const double* hi,
                                                const double* origin, const double* period);
GPDE_API int gpde_radius_csr_periodic_count(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                                   double r, uint32_t flags, const double* lo, const double* hi, const double* origin,
                                   const double* period, int32_t* deg, void* ws, size_t ws_bytes, void* stream);
GPDE_API int gpde_radius_csr_periodic_fill(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                                  double r, uint32_t flags, const double* lo, const double* hi, const double* origin,
                                  const double* period, const int32_t* rowptr, int32_t* src, int32_t* dst, float* geom,
                                  int64_t n_edges, void* ws, size_t ws_bytes, void* stream);

/* The cell-list builder for a BATCH of independent point sets: the block-diagonal destination CSR of B radius graphs in one
 * build (what a DataLoader makes of the per-sample graphs of the reference's training scripts, UAI3_resolution.py:131-145,
 * neurips1_MGKN.py:204 - one ball_connectivity per sample - without one build per sample).  Graph b owns the sources
 * ptr_src[b] .. ptr_src[b + 1] and the destinations ptr_dst[b] .. ptr_dst[b + 1] of the concatenated position arrays and has
 * its own radius r[b]; node ids in rowptr / src / dst are GLOBAL (rows of the concatenated destinations, sources of the
 * concatenated sources).  Rows as in the open builder: ascending source id (rows longer than 4096 edges keep cell order),
 * self-loops included, both arithmetics (flags as gpde_radius_csr_count; under GPDE_RADIUS_REFERENCE_TIES the forced zero of
 * the diagonal compares global ids).  pos_dst == pos_src with n_dst == n_src means ONE point set (then ptr_dst = ptr_src).
 *   gpde_radius_csr_batched_plan   HOST ONLY, no device call.  bounds [B][2][dim]: lo then hi of a box around both point sets of
 *       graph b (not read for a graph without sources, which gets one empty cell, as does a graph of coincident points);
 *       ptr_src / ptr_dst [B + 1] (ptr_dst NULL = ptr_src); r [B].  Writes B records of GPDE_RADIUS_BATCHED_REC_BYTES bytes
 *       into the host array `table` (NULL: a query) - each graph's own cell grid by the rule of the open builder, its radius
 *       terms, its first cell in the batch-wide numbering and its point ranges - and returns the summed cell count and the
 *       workspace bytes of count / fill.  The summed cell count is held to 2^24: while it is exceeded every graph's cell edge
 *       doubles (the grid is only a filter: the edges do not depend on it); more graphs than that end at one cell each.
 *   gpde_radius_csr_batched_count / _fill   the two passes with the caller's scan between them, `ws` untouched in between, like
 *       the open twins.  `table`: the planned records in a DEVICE buffer (the caller uploads them; the library copies nothing
 *       between host and device); n_cells: what the plan returned.  ptr_src / ptr_dst are the HOST arrays again, checked on
 *       every call; the records must be the plan of these very arrays.
 * GPDE_EINVAL with a gpde_last_error() text, before any device call, for: dim outside 1..3; n_graphs < 0; a ptr array that is
 * NULL, does not start at 0, decreases, or does not end at the point count (at most 2^31 - 1); r[b] not positive and finite;
 * unknown flags; null positions, table, deg, rowptr, src / dst or ws; n_cells < n_graphs.  GPDE_EWORKSPACE for a short workspace.
 * n_graphs = 0 and zero points are valid calls.  Additions to the ABI: GPDE_VERSION is unchanged. */
enum { GPDE_RADIUS_BATCHED_REC_BYTES = 96 };
GPDE_API int gpde_radius_csr_batched_plan(const double* bounds, const int64_t* ptr_src, const int64_t* ptr_dst, const double* r,
                                 int64_t n_graphs, int dim, void* table, int64_t* n_cells, size_t* ws_bytes);
GPDE_API int gpde_radius_csr_batched_count(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                                  uint32_t flags, const int64_t* ptr_src, const int64_t* ptr_dst, int64_t n_graphs,
                                  const void* table, int64_t n_cells, int32_t* deg, void* ws, size_t ws_bytes, void* stream);
GPDE_API int gpde_radius_csr_batched_fill(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                                 uint32_t flags, const int64_t* ptr_src, const int64_t* ptr_dst, int64_t n_graphs,
                                 const void* table, int64_t n_cells, const int32_t* rowptr, int32_t* src, int32_t* dst,
                                 int64_t n_edges, void* ws, size_t ws_bytes, void* stream);

/* CAP A GRAPH'S IN-DEGREE: per destination row of a CSR keep the k in-edges of smallest key (gpde_select.hip).  The builders
 * above emit the full ball of every destination and nothing bounds a row; the method itself estimates the kernel integral from
 * m points of the ball (Nystrom), the reference's mesh generators offer a thinned connectivity next to ball_connectivity
 * (gaussian_connectivity, graph-neural-operator utilities.py:257-263, 372-378) and PyG's radius_graph has max_num_neighbors.
 * The selection works on a finished CSR - any builder's, or gpde_csr_from_coo's.
 *   gpde_csr_select_k   rowptr int32 [n_rows + 1], keys int64 [n_edges] by CSR slot, k >= 1.  A row of at most k in-edges is kept
 *       whole; a longer row keeps the k slots with the smallest (key, slot) in lexicographic order (slots are distinct: the choice
 *       is unique).  rowptr_out int32 [n_rows + 1] is GIVEN by the caller - the exclusive scan of min(deg, k) - and n_out is its
 *       total; slots_out int32 [n_out] receives the kept INPUT slots, ascending inside every row: source order, and with it the
 *       operator's summation order, is preserved.  No atomics: two identical calls give identical bits.  The selection for k is a
 *       subset of the selection for any k' > k.  One wave per row finds the k-th smallest key by bisection over the key bits and
 *       emits in one pass in slot order; rows of up to 2048 keys are staged in LDS, longer ones are re-read.  Any row length.
 *   gpde_edge_keys_sqdist   keys[s] = the IEEE-754 bits of the float64 squared distance of edge (src[s] in pos_src -> dst[s] in
 *       pos_dst) - a non-negative double orders as its int64 bits.  Open axes: d = pos_dst[i][a] - pos_src[j][a], d2 += d * d in
 *       axis order, contraction off: the arithmetic of gpde_radius_csr_* (flags = 0), so a float64 host computation reproduces
 *       the bits.  period / origin: HOST arrays [dim] as in gpde_radius_csr_periodic_* (period[a] = 0: an open axis), or NULL (no
 *       periodic axis / origin 0): on a periodic axis d = pos_src[j][a] - pos_dst[i][a], d -= L rint(d / L) on the RAW
 *       coordinates (L = period[a]; rint rounds half to even) - the minimum-image difference in the form a float64 host
 *       computation follows operation by operation; it does not depend on the origin, which is only checked.  (The periodic
 *       BUILDER reduces both points into [origin, origin + L) and subtracts an image x_d +- L: the same distance up to rounding,
 *       tens of ulp apart in d2 for an edge that crosses the seam.)  The node ids of src / dst are NOT checked
 *       against the point counts (the call does not see them): they are a CSR's, built for these point sets.
 *   gpde_edge_keys_hash     keys[s] = a counter-based hash of (seed, dst_ids[s], src_ids[s]) - independent of slot order, of the
 *       builder and of k; the ids are explicit int32 arrays so that a batch can pass graph-local ids.  All arithmetic mod 2^64
 *       (the constants below ARE the specification; seed is the int64 reinterpreted as uint64):
 *           z = seed * GPDE_HASH_SEED_MUL + ((uint64)dst << 32 | (uint64)src)
 *           z = (z ^ z >> 30) * GPDE_HASH_MUL1;   z = (z ^ z >> 27) * GPDE_HASH_MUL2;   z ^= z >> 31;   key = (int64)(z >> 1)
 *       A uniform k-subset of the ball under aggr = mean is the UNBIASED Monte-Carlo estimate of the full-ball mean; the k
 *       nearest are not (they sample the inner part of the ball only).
 * Zero rows and zero edges are valid calls.  GPDE_EINVAL with a gpde_last_error() text, before any device call, for NULL
 * arguments, k < 1, sizes outside an int32 CSR and an n_out that cannot be the total of rowptr_out (negative, or more than
 * min(n_edges, n_rows * k); rowptr_out is device memory and no call here synchronises, so the exact total is the caller's word -
 * the kernel writes no slot at or past n_out whatever rowptr_out holds); GPDE_EUNSUPPORTED for dim outside 1..3.
 * Additions to the ABI: GPDE_VERSION is unchanged. */
#define GPDE_HASH_SEED_MUL 0x9E3779B97F4A7C15ull
#define GPDE_HASH_MUL1 0xBF58476D1CE4E5B9ull
#define GPDE_HASH_MUL2 0x94D049BB133111EBull
GPDE_API int gpde_csr_select_k(const int32_t* rowptr, const int64_t* keys, int64_t n_rows, int64_t n_edges, int64_t k,
                      const int32_t* rowptr_out, int32_t* slots_out, int64_t n_out, void* stream);
GPDE_API int gpde_edge_keys_sqdist(const double* pos_src, const double* pos_dst, int dim, const double* period,
                          const double* origin, const int32_t* src, const int32_t* dst, int64_t n_edges, int64_t* keys,
                          void* stream);
GPDE_API int gpde_edge_keys_hash(const int32_t* src_ids, const int32_t* dst_ids, int64_t n_edges, int64_t seed,
                        int64_t* keys, void* stream);

/* EXACT K-NEAREST-NEIGHBOUR GRAPHS as the destination CSR (gpde_knn.hip): the counterpart of PyG's knn_graph / knn, built
 * without a radius - the selection above needs a ball that holds k sources around EVERY destination, formed in full first.
 * Sources pos_src float64 [n_src][dim], destinations pos_dst float64 [n_dst][dim], dim 1..3 (device arrays).  ONE point set is
 * the call with pos_src == pos_dst and n_src == n_dst.  Row i holds the k_eff sources j with the smallest (d2_bits(j, i), j) in
 * lexicographic order:
 *   d2_bits   the int64 bit pattern of the float64 squared distance in the open-axis arithmetic of gpde_edge_keys_sqdist:
 *             d = pos_dst[i][a] - pos_src[j][a], d2 += d * d in axis order, contraction off.  Ties go to the smaller source id;
 *   loop      0 on one point set: the pair j == i is excluded BY ID (another point at distance 0 is an ordinary candidate);
 *             1, or two point sets: nothing is excluded;
 *   k_eff     min(k, n_src); with loop = 0 on one point set min(k, n_src - 1).  It is the same for every row:
 *             rowptr[i] = i * k_eff (written by the call), n_edges = n_dst * k_eff - the caller sizes src / dst (int32 [n_edges])
 *             and geom before the call, and nothing has to be read back;
 *   rows      ascending source id inside a row (the Csr convention: it fixes the operator's summation order); perm = identity.
 * That is gpde_csr_select_k applied to the complete bipartite graph under gpde_edge_keys_sqdist keys (self pairs dropped first
 * for loop = 0).  The graph is a pure function of the positions, k and loop: not of the cell edge, the box, the launch geometry
 * or call history; no atomics; two calls give identical bits.  Non-finite positions give unspecified edges (valid ids, no
 * out-of-bounds access, no unbounded loop).
 *   lo / hi   HOST arrays [dim]: the box the cell grid covers.  Points outside it are binned into the border cells: any finite
 *             box with hi >= lo gives the same graph, a box around both point sets the fastest build.
 *   cell      the cell edge; 0: automatic - a mean occupancy of max(2, k / 2) sources per cell, over the axes that have extent
 *             (gpde_knn.hip knn_auto_cell).  Edges that give more than 2^16 cells on an axis or 2^24 in all are doubled until
 *             they fit.  It changes the speed, never the result.
 *   geom      nullable; float32 [n_edges][dim + 1] by CSR slot: pos_src[src] - pos_dst[dst] per axis and its norm, float64
 *             rounded once - the values of gpde_radius_csr_periodic_fill on open axes for the same edge.
 *   ws        gpde_knn_csr_workspace_bytes(...) bytes (host arithmetic only; 0 and gpde_last_error() for what it can refuse).
 * gpde_knn_csr launches on `stream`, never synchronises and never allocates.  Before any device call: GPDE_EUNSUPPORTED for dim
 * outside 1..3; GPDE_EINVAL for k < 1, k > GPDE_KNN_MAX_K, loop not 0 or 1, point counts outside 0 .. 2^31 - 1,
 * n_dst * k_eff outside an int32 CSR, a cell that is negative, not finite or has no finite reciprocal, NULL lo / hi, a box that is not finite or has hi < lo, NULL
 * positions of a non-empty set, NULL rowptr / ws, NULL src / dst with n_edges > 0; GPDE_EWORKSPACE for a short workspace.
 * Zero sources and zero destinations are valid calls.  Additions to the ABI: GPDE_VERSION is unchanged. */
#define GPDE_KNN_MAX_K 256
GPDE_API size_t gpde_knn_csr_workspace_bytes(int64_t n_src, int64_t n_dst, int dim, int64_t k, double cell, const double* lo,
                                    const double* hi);
GPDE_API int gpde_knn_csr(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim, int64_t k,
                 int loop, double cell, const double* lo, const double* hi, int32_t* rowptr, int32_t* src, int32_t* dst,
                 float* geom, void* ws, size_t ws_bytes, void* stream);

/* The nearest-neighbour builder for a BATCH of independent point sets (gpde_knn_arms.hip): the block-diagonal destination CSR of
 * B kNN graphs in one build - what a DataLoader makes of per-sample knn graphs - without one build per sample.  Graph b owns the
 * sources ptr_src[b] .. ptr_src[b + 1] and the destinations ptr_dst[b] .. ptr_dst[b + 1] of the concatenated float64 position
 * arrays; node ids in rowptr / src / dst are GLOBAL.  ptr_dst = NULL, or pos_dst == pos_src with n_dst == n_src (then ptr_dst must
 * repeat ptr_src), is ONE point set per graph.
 *   k_eff[b]  min(k, ns_b); with loop = 0 (one point set: the pair of equal id is excluded) min(k, ns_b - 1), never negative: a
 *             graph with destinations but no usable source has empty rows.  loop = 0 with two point sets is refused (pass 1);
 *   slots     edge_ptr[b + 1] = edge_ptr[b] + nd_b k_eff[b]; row i of graph b starts at rowptr[i] = edge_ptr[b] + (i - ptr_dst[b])
 *             k_eff[b].  All of it is host arithmetic on the ptr arrays: n_edges = edge_ptr[B] is known before anything runs (the
 *             plan returns it) and the call writes rowptr itself;
 *   result    rowptr / src / dst / geom are the per-graph gpde_knn_csr results concatenated with their offsets, BIT FOR BIT: keys
 *             and ties are the open arm's, evaluated inside the destination's own graph - a source of another graph is never a
 *             candidate, however the graphs overlap in space.  No atomics; two calls give identical bits.
 *   gpde_knn_csr_batched_plan   HOST ONLY, no device call.  bounds [B][2][dim]: lo then hi of a box of graph b (not read for a
 *       graph without sources, which gets one cell, as does a graph of coincident points); `cell`: every graph's cell edge, 0 =
 *       automatic per graph (the open arm's rule with that graph's ns_b and box).  Writes B records of
 *       GPDE_KNN_BATCHED_REC_BYTES bytes into the host array `table` (NULL: a query) and returns the summed cell count, the
 *       workspace bytes and n_edges.  The summed cell count is held to 2^24 by doubling every graph's cell edge: the grid
 *       changes the speed, never the result.
 *   gpde_knn_csr_batched   `table`: the planned records in a DEVICE buffer (the caller uploads them); n_cells, n_edges: what the
 *       plan returned; ptr_src / ptr_dst the HOST arrays again.  Launches on `stream`; never synchronises, never allocates.  The
 *       LDS buffer of a wave is sized by max_b k_eff[b].
 * Before any device call: GPDE_EUNSUPPORTED for dim outside 1..3; GPDE_EINVAL for k outside 1 .. GPDE_KNN_MAX_K, loop not 0 or 1,
 * a bad cell, n_graphs < 0, a ptr array that is NULL, does not start at 0, decreases or does not end at the point count, a box
 * of a graph with sources that is empty or not finite, NULL arguments, n_edges that is not the plan's or lies outside the int32
 * CSR; GPDE_EWORKSPACE for a short workspace.  n_graphs = 0 and zero points are valid calls.  GPDE_VERSION is unchanged. */
enum { GPDE_KNN_BATCHED_REC_BYTES = 128 };
GPDE_API int gpde_knn_csr_batched_plan(const double* bounds, const int64_t* ptr_src, const int64_t* ptr_dst, int64_t n_graphs, int dim,
                              int64_t k, int loop, double cell, void* table, int64_t* n_cells, size_t* ws_bytes, int64_t* n_edges);
GPDE_API int gpde_knn_csr_batched(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim, int64_t k,
                         int loop, const int64_t* ptr_src, const int64_t* ptr_dst, int64_t n_graphs, const void* table,
                         int64_t n_cells, int32_t* rowptr, int32_t* src, int32_t* dst, float* geom, int64_t n_edges, void* ws,
                         size_t ws_bytes, void* stream);

/* The nearest-neighbour builder on a TORUS (gpde_knn_arms.hip): gpde_knn_csr with the minimum-image distance.  period / origin:
 * HOST arrays [dim] (origin NULL: 0).  period[a] > 0: axis a wraps with that length; period[a] == 0: an open axis.  Points
 * anywhere on the real line are legal on a periodic axis.  origin only anchors the cell grid: the graph does not depend on it.
 *   key       the int64 bit pattern of the float64 squared distance in the periodic arithmetic of gpde_edge_keys_sqdist: on a
 *             periodic axis d = pos_src[j][a] - pos_dst[i][a], d -= L rint(d / L) on the RAW coordinates (half to even); on an
 *             open axis the plain difference; squares summed in axis order, contraction off.  Ties go to the smaller source id.
 *             Every source is a candidate once, at its minimum image: a row never holds a source twice;
 *   k_eff, rowptr, rows, loop   as gpde_knn_csr.  There is no 2 r < period precondition: k may reach every source on the torus.
 * That is gpde_csr_select_k on the complete bipartite graph under gpde_edge_keys_sqdist(period) keys - a pure function of the
 * positions, k, loop and period: not of origin, the cell edge, lo / hi or call history.
 *   geom      nullable; float32 [n_edges][dim + 1]: the per-axis d of the key (source minus target, on an open axis
 *             pos_src - pos_dst) and sqrt of their squares' sum, float64 rounded once.  NOT the arithmetic of
 *             gpde_radius_csr_periodic_fill, which reduces both points into the box first and is undefined at separations of
 *             period / 2 and beyond; the two agree up to their last bits where both exist;
 *   lo / hi   read on OPEN axes only (NULL when every axis is periodic); cell: as gpde_knn_csr - a periodic axis is tiled by
 *             floor(period / cell) cells.
 * Refusals as gpde_knn_csr, and GPDE_EINVAL for a NULL period, a negative or non-finite period (or one without a finite
 * reciprocal) and a non-finite origin.  Never synchronises, never allocates.  GPDE_VERSION is unchanged. */
GPDE_API size_t gpde_knn_csr_periodic_workspace_bytes(int64_t n_src, int64_t n_dst, int dim, int64_t k, double cell, const double* lo,
                                             const double* hi, const double* origin, const double* period);
GPDE_API int gpde_knn_csr_periodic(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim, int64_t k,
                          int loop, double cell, const double* lo, const double* hi, const double* origin, const double* period,
                          int32_t* rowptr, int32_t* src, int32_t* dst, float* geom, void* ws, size_t ws_bytes, void* stream);

/* SAMPLED GRAPHS: the reference's second connectivity, gaussian_connectivity (graph-neural-operator utilities.py:257-263,
 * 372-378; multipole-graph-neural-operator utilities.py:283-289, 419-425), built natively as the destination CSR (the sampled
 * arm of gpde_cellgraph.hip).  The edge j -> i (j in pos_src, i in pos_dst; level-local ids) is kept iff
 *       u(seed, i, j) < exp(-(d2 / (sigma * sigma)))                          float64, round to nearest, nothing fused
 *   u   ((double)(key >> 10) + 0.5) * 2^-53 with key = what gpde_edge_keys_hash gives for (seed, dst = i, src = j): the 53 top
 *       bits of the mix, at the centre of their cell (the sum is rounded like any float64 sum); 2^-54 <= u.
 *   d2  what gpde_edge_keys_sqdist gives for the edge, bit for bit (open axes d = x_dst - x_src; periodic axes d = x_src - x_dst,
 *       d -= L rint(d / L) on the raw coordinates; squares summed in axis order).
 * The graph is a pure function of positions, sigma and seed - not of cells, waves or call history; the two directions of a pair
 * are independent draws; a pair at d = 0 (a point with itself) has p = 1 and is kept.  Since u >= 2^-54 no pair with
 * exp(-d2 / sigma^2) <= 2^-54 is kept: the graph lies inside the radius graph of r_support = sigma sqrt(54 ln 2) ~ 6.118 sigma, and
 * the cell list (cells of edge >= min(r_support, cutoff)) is exact.  The kernel skips exp where the binary exponent of u
 * against d2 / sigma^2 decides; the kept set is the predicate's.  A host that follows the formula differs only where its exp and
 * the device's differ in the last places AND u lies between them.
 *   cutoff   0: none.  > 0: additionally drops every pair with d2 > cutoff * cutoff - a TRUNCATED Gaussian, another graph.
 *   origin / period   HOST arrays [dim] as in gpde_radius_csr_periodic_* (NULL: origin 0 / no periodic axis).  A periodic axis needs
 *            2 min(r_support, cutoff) < period[k].  lo / hi: HOST arrays [dim], a bounding box of both point sets, read on open axes.
 *   geom (fill, nullable)   float32 [E][dim + 1] by CSR slot, the values of gpde_radius_csr_periodic_fill for the edge.
 *   max_in_degree (fill)    the largest entry of COUNT's `deg`, or 0 when the caller does not know it.  It only sizes the LDS row
 *            sort (the smallest power of two >= it, 64 .. 4096 slots per wave; 0: 4096) and with it the waves in flight; a value
 *            below the true one leaves the rows longer than that power of two in cell order instead of ascending.
 * Two passes with the caller's scan between them, `ws` untouched in between, like the radius builders; rows in ascending source
 * order (rows longer than 4096 edges keep cell order); no atomics, COUNT and FILL evaluate the same predicate.  Before any device
 * call: GPDE_EUNSUPPORTED for dim outside 1..3; GPDE_EINVAL for sigma (or sigma^2) not positive and finite, a negative or
 * non-finite cutoff, a bad period / origin, the periodic rule, NULL positions / deg / rowptr / src / dst / ws, negative sizes and
 * n_edges outside an int32 CSR; GPDE_EWORKSPACE for a short workspace; the workspace query returns 0 for what it can see.
 * Additions to the ABI: GPDE_VERSION is unchanged. */
GPDE_API size_t gpde_gaussian_csr_workspace_bytes(int64_t n_src, int dim, double sigma, double cutoff, const double* lo,
                                         const double* hi, const double* origin, const double* period);
GPDE_API int gpde_gaussian_csr_count(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                            double sigma, double cutoff, int64_t seed, const double* lo, const double* hi, const double* origin,
                            const double* period, int32_t* deg, void* ws, size_t ws_bytes, void* stream);
GPDE_API int gpde_gaussian_csr_fill(const double* pos_src, int64_t n_src, const double* pos_dst, int64_t n_dst, int dim,
                           double sigma, double cutoff, int64_t seed, const double* lo, const double* hi, const double* origin,
                           const double* period, const int32_t* rowptr, int32_t* src, int32_t* dst, float* geom,
                           int64_t n_edges, int64_t max_in_degree, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GCNConv (gpde_gcn.hip): the graph convolution of Kipf & Welling, the baseline network of the multipole paper
 * (multipole-graph-neural-operator/neurips4_GCN.py:28-31 `GCNConv(width, width)`, applied 16 times per forward), on the
 * destination CSR of gpde_csr_from_coo.  Square graphs (one node set).
 *   gpde_gcn_norm   PyG's `gcn_norm` with `add_remaining_self_loops`.  edge_weight [E] in ORIGINAL edge order (read through perm;
 *       NULL: every weight 1; perm NULL: slot order).  With GPDE_GCN_NORMALIZE | GPDE_GCN_ADD_SELF_LOOPS every node gets exactly
 *       one self loop of weight `fill` (2 with GPDE_GCN_IMPROVED, else 1); a node that already has self-loop edges takes the
 *       weight of the one with the largest original edge id instead, and every self-loop SLOT gets coef = 0.  deg[i] = sum of w
 *       over the other in-edges of i + the self weight - the TARGET-side degree of PyG >= 1.6 (older releases summed over the
 *       source row: the same number on a symmetric graph) - summed per row in ascending slot order in float64, no atomics.
 *       dinv = deg^-1/2 (0 where deg == 0; 1 / sqrt in float64), coef[slot] = dinv[src] w dinv[dst], self_coef[i] = dinv[i]^2 *
 *       self weight.  NORMALIZE without ADD_SELF_LOOPS: no self term (self_coef = 0), existing self loops are ordinary edges.
 *       Without NORMALIZE: coef = w, self_coef = 0 (GPDE_GCN_IMPROVED / ADD_SELF_LOOPS are then without effect).
 *       coef [E] by CSR slot and self_coef [N] are overwritten.  Workspace: gpde_gcn_norm_workspace_bytes.
 *   gpde_gcn_fwd    out[i] = (sum_{e -> i} coef[e] x[src[e]] + self_coef[i] x[i]) . W + bias        x [N][in], W [in][out] row-major,
 *       out [N][out].  W == NULL: the aggregation alone (out_channels must equal in_channels); bias [out], self_coef [N] and
 *       agg_out nullable; agg_out [N][in] receives the aggregated rows BEFORE the multiply (the backward's A^T g, from which
 *       grad_W = x^T . agg_out follows).  flags: GPDE_GCN_RELU clamps the result at 0.  out / agg_out must not overlap x or each
 *       other.  Aggregation first, then the multiply on the exact fp32 MFMA while the tile is in LDS; rows summed two-level (chains
 *       of 64 in-edges); no atomics - two calls give the same bits.
 *   gpde_gcn_plan   HOST ONLY: the launcher's tiling at these widths - out[0..7] = destination rows per workgroup, LDS row stride
 *       (floats), channel passes per lane of the aggregation (ceil(in / 64)), 32-column blocks of the product, column blocks per
 *       wave, K tail (in odd), column tail (out % 32 != 0), LDS bytes.
 * 1 <= in_channels, out_channels <= GPDE_WECONV_ANY_MAX_WIDTH; other widths, NULL arrays, unknown flags: GPDE_EINVAL with a
 * gpde_last_error() text before any device work.  n_nodes == 0 is a valid call that reads no pointer; with n_edges == 0 src,
 * perm, edge_weight and coef may be NULL.  Additions to the ABI: GPDE_VERSION is unchanged. */
enum { GPDE_GCN_ADD_SELF_LOOPS = 1, GPDE_GCN_IMPROVED = 2, GPDE_GCN_NORMALIZE = 4 /* gpde_gcn_norm flags */ };
enum { GPDE_GCN_RELU = 1 /* gpde_gcn_fwd flags */ };
GPDE_API size_t gpde_gcn_norm_workspace_bytes(int64_t n_nodes, int64_t n_edges);
GPDE_API int gpde_gcn_norm(const int32_t* rowptr, const int32_t* src, const int32_t* perm, const float* edge_weight, int64_t n_nodes,
                  int64_t n_edges, uint32_t flags, float* coef, float* self_coef, void* ws, size_t ws_bytes, void* stream);
GPDE_API int gpde_gcn_fwd(const float* x, int64_t n_nodes, int64_t n_edges, const int32_t* rowptr, const int32_t* src,
                 const float* coef, const float* self_coef, const float* W, const float* bias, int in_channels, int out_channels,
                 uint32_t flags, float* out, float* agg_out, void* stream);
GPDE_API int gpde_gcn_plan(int in_channels, int out_channels, int32_t* out);

/* The DIAGONAL-kernel operator (gpde_diagconv.hip): the reference's `NNConv` / `NNConv_Gaussian` (nn_conv.py:8-96, 99-194), whose
 * kernel emits `width` values per edge that diag_embed makes a diagonal width x width matrix - the message is x_j (.) k_e:
 *     out_i = aggr_{e: j -> i} x_src[j] (.) k_e  +  x_dst[i] . root + bias  (+ residual, ReLU)
 *   x_src [n_src][width] is what the edges gather, k [E][width] fp32 in CSR slot order, x_dst [n_dst][in_dst] (nullable: no root
 *   term) and root [in_dst][width] (nullable) enter the root term only, bias [width] and residual [n_dst][width] nullable (residual
 *   must not be out), out [n_dst][width].  A call on ONE node set hands one table twice (x_dst = x_src, n_dst = n_src, in_dst =
 *   width).  aggr add / mean / max in the forward (mean divides by clamp(count, 1); a destination without in-edges aggregates to 0,
 *   also for max), add / mean in the backward (GPDE_AGGR_MAX: GPDE_EUNSUPPORTED - its gradient is composed by the caller).
 *   gpde_diagconv_bwd   (outputs overwritten, NULL skips the term)
 *       grad_k [E][width]            = x_j (.) gT_i, gT_i = g_i (/ clamp(deg_i, 1) for mean); needs src and x_src
 *       grad_x_src [n_src][width]    = sum_{e: j ->} k_e (.) gT_dst(e), ONE owner per source in ascending slot order over src_rowptr /
 *                                      src_slots (gpde_csr_source_order over n_src) - required with it when n_edges > 0, as are k
 *                                      and dst [E] (the destination of each CSR slot); never atomics
 *       grad_x_dst [n_dst][in_dst]   = g . root^T (0 without root).  One node set - x_dst == x_src (the same address), n_dst == n_src,
 *                                      in_dst == width and grad_x_dst == NULL: that term is ADDED to grad_x_src instead
 *       grad_root [in_dst][width]    = x_dst^T g,  grad_bias [width] = colsum g (ordered strips)
 *       ws: gpde_diagconv_bwd_workspace_bytes(n_dst, width, in_dst) bytes (gT for mean, the strip partials).
 *   gpde_diagconv_plan  HOST ONLY, from the function the launchers call: out[0..9] = V (floats per access: 4 when vec4 != 0 and
 *       width % 4 == 0, else 1), LC (column lanes, a power of two), ES (edge slots per wave = 64 / LC), in-edges per pass (their
 *       loads are in flight before the first FMA), in-edges per chain (first level of the two-level row sum), LC * ES, channels per
 *       column lane, 1 when a lane's channels are consecutive (width % 4 == 0: 4 lc .. 4 lc + 3, read by one 16-byte or four dword
 *       accesses) and 0 when strided by LC, lanes that own a channel, LDS bytes.  The tiling and the summation order depend on
 *       width alone: an unaligned buffer changes the instructions (V), not the bits.
 * Plain fp32 fmaf, no atomics, every sum in an order fixed by the graph: two calls give the same bits.  1 <= width, in_dst <=
 * GPDE_WECONV_ANY_MAX_WIDTH, else GPDE_EUNSUPPORTED.  GPDE_EINVAL with a gpde_last_error() text, before any device call, for NULL
 * required pointers, an unknown aggr, edges without sources or destinations, root without x_dst, residual == out and an out that
 * overlaps x_src (other waves still gather those rows).  Zero nodes
 * and zero edges are valid calls.  Additions to the ABI: GPDE_VERSION is unchanged. */
GPDE_API int gpde_diagconv_plan(int width, int vec4, int aggr, int32_t* out);
GPDE_API int gpde_diagconv_fwd(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst, const float* k, int64_t n_edges,
                      const int32_t* rowptr, const int32_t* src, const float* root, const float* bias, const float* residual,
                      int relu, int aggr, int width, int in_dst, float* out, void* stream);
GPDE_API size_t gpde_diagconv_bwd_workspace_bytes(int64_t n_dst, int width, int in_dst);
GPDE_API int gpde_diagconv_bwd(const float* x_src, int64_t n_src, const float* x_dst, int64_t n_dst, const float* k, int64_t n_edges,
                      const int32_t* rowptr, const int32_t* src, const int32_t* dst, const int32_t* src_rowptr,
                      const int32_t* src_slots, const float* root, int aggr, int width, int in_dst, const float* grad_out,
                      float* grad_x_src, float* grad_x_dst, float* grad_k, float* grad_root, float* grad_bias, void* ws,
                      size_t ws_bytes, void* stream);

/* HIP-event timing of the kernels launched by gpde_nnconv_fwd on the calling thread (used by
 * bench.py for the roofline figure; events are recorded on the same stream as the kernels).
 * gpde_profile_begin() arms it; gpde_profile_end_kinds() disarms it, SYNCHRONISES on the recorded
 * events and returns the summed duration (ms) and launch count per kernel kind: ms_by_kind / launches_by_kind are arrays of
 * GPDE_PROF_KINDS entries.  Not for production calls. */
GPDE_API int gpde_profile_begin(void);
enum {
    GPDE_PROF_FUSED = 0,     /* fused edge kernel (gpde_nnconv_fwd_kernel names it) or gpde_zagg_kernel */
    GPDE_PROF_GEMM3 = 1,     /* per-node last Linear Z . W3 */
    GPDE_PROF_EPILOGUE = 2,  /* split-K sum, b3, mean, x . root + bias */
    GPDE_PROF_PREP = 3,      /* pre-passes of the split-f16 aggregation (3 tiny kernels + memset) */
    GPDE_PROF_OTHER = 4,
    GPDE_PROF_KINDS = 5
};
GPDE_API int gpde_profile_end_kinds(double* ms_by_kind, int32_t* launches_by_kind);

/* Which branches the native backward took (tests).  gpde_bwd_trace_begin() arms a trace on the calling thread and empties it;
 * while it is armed every gpde_nnconv_bwd / _light / _deferred / gpde_hidden_bwd call appends one record of
 * GPDE_BWD_TRACE_FIELDS int32 per chunk it processes (node-aligned chunks; the edge chunks of gpde_hidden_bwd with na = nb = -1).
 * Each field is written where the backward takes that decision.  gpde_bwd_trace_end() disarms it, copies up to `capacity` records
 * to `records`, writes the number recorded to *n_records and empties the trace.  Host only, no device work; unarmed, a call pays
 * one thread-local read. */
GPDE_API int gpde_bwd_trace_begin(void);
GPDE_API int gpde_bwd_trace_end(int32_t* records, int32_t capacity, int32_t* n_records);
enum {
    GPDE_BWD_TRACE_PHASE = 0,       /* 0 full, 1 conv (given H, dL/dU written), 2 mlp (gpde_hidden_bwd), 3 light, 4 deferred */
    GPDE_BWD_TRACE_NA = 1,          /* first node of the chunk */
    GPDE_BWD_TRACE_NB = 2,          /* one past its last node */
    GPDE_BWD_TRACE_E0 = 3,          /* first CSR slot */
    GPDE_BWD_TRACE_ROWS = 4,        /* edges (CSR slots) of the chunk */
    GPDE_BWD_TRACE_EDGE_KERNEL = 5, /* 0 none, 1 gpde_edge_bwd_kernel, 2 gpde_edge_bwd2_kernel, 3 gpde_edge_bwd3_kernel (split f16) */
    GPDE_BWD_TRACE_Z = 6,           /* source of Z: 0 none, 1 kept by the forward, 2 gpde_zagg_kernel (fp32), 3 gpde_zagg_kernel<true> */
    GPDE_BWD_TRACE_HLAST = 7,       /* last hidden layer: 0 not needed, 1 given, 2 fused store kernel, 3 the layer loop */
    GPDE_BWD_TRACE_H1 = 8,          /* H_1: 0 not formed here, 1 fp32 GEMM, 2 k_first_layer, 3 on the fly (never written) */
    GPDE_BWD_TRACE_CALL_AMAX = 9,   /* 1: one attribute bound per slot for the whole call */
    GPDE_BWD_TRACE_DU1 = 10,        /* dU_1: 0 not formed, 1 split-f16 NT GEMM, 2 fp32 GEMM */
    GPDE_BWD_TRACE_DW2 = 11,        /* dW_2: 0 not formed, 1 split-f16 TN GEMM, 2 gemm_tn_acc */
    GPDE_BWD_TRACE_DW1 = 12,        /* dW_1, db_1: 0 not formed, 1 dU_1 GEMM epilogue, 2 k_dw_first, 3 gemm_tn_acc */
    GPDE_BWD_TRACE_DU_PRE = 13,     /* 1: the per-edge kernel left dU_2^T, its row scales and tile column partials */
    GPDE_BWD_TRACE_ORDERED = 14,    /* 1: grad_x summed per source in slot order (k_dx_reduce); 0: atomics */
    GPDE_BWD_TRACE_GRAD_ATTR = 15,  /* 1: dL/d edge_attr formed (k_grad_attr) */
    GPDE_BWD_TRACE_FROM_H = 16,     /* 1: the chunk read last hidden activations the caller gave (hidden_saved, a partial H, the
                                       `hidden` form) instead of recomputing them */
    GPDE_BWD_TRACE_FIELDS = 17
};

#ifdef __cplusplus
}
#endif
#endif /* GPDE_H */
