// Fused edge kernel, f16-split, ONE WAVE PER SIMD with a 512-register budget (v6, the default for
// graphs from 32,768 edges on): 4 waves per workgroup, wave tile = 64 edges x 128 hidden columns.
//
// Same contract and math as gpde_fused_f16v3_kernel<false, true, false> (gpde_fused_f16v3.hip; replaces
// the hidden part of DenseNet.forward, /root/reference/graph-neural-operator/utilities.py:223-227,
// NNConv_old.message, nn_conv.py:273-275, and PyG's gather / scatter): per edge
//   H1 = relu((W1|b1) . attr)  ->  H2 = relu(W2 . H1 + b2)  ->  Z_dst[c][k] += x_src[c] * H2[k]
// with the k1 x k2 layer and the aggregation on 2-term split f16 MFMA, fp32 accumulation.
//
// Why this shape (scripts/ubench/kloop_model_v6.hip, measured on MI355X; DESIGN.md §3d has the figures; the 8-wave v3
// kernel sits at 51 % matrix-pipe occupancy):
//   * the v3 kernel's two waves per SIMD both convert the same H1 tile, share the SIMD's issue port and
//     lose ~40 % of the loop to conversions, barrier waits and staging.  One wave per SIMD with a wave
//     tile twice as tall halves conversions, W2 fragment reads, DMA pieces and barriers per MFMA;
//   * 512 registers: accumulators (128) and Z (128) live in AGPRs for the whole kernel, nothing spills
//     (v3: 256 registers, 50 spilled);
//   * every MFMA is v_mfma_f32_16x16x32_f16.  Under load this chip holds its clock down, and how far depends on the MFMA
//     shape: the K loop on 32x32x16 ran at 1.9-2.0 GHz, the same tile and the same FLOP on 16x16x32 run at 2.36 GHz (the
//     model's bare streams: 1.6 against 2.05 GHz).  Layout: lane l = (l15 = l % 16, g = l / 16).  A and B operands: row /
//     column l15, k slots 8g .. 8g+7;  C / D: column l15, rows 4g .. 4g+3.  acc = 4 edge blocks x 8 column blocks of
//     f32x4, Z = 4 channel blocks x 8 column blocks.  The W2 chunk image of gpde_pack.hip is read as it is (lane group g
//     takes unit g: one ds_read_b128 for hi, one for lo, conflict-free within 16 lanes); H1 takes ONE MFMA per 16 rows x
//     16 edges, its three split terms in the lane groups of K = 32, with the (W1|b1) rows picked by LDS address so that
//     the result is the hidden layer's A operand without a cross-lane move; the aggregation covers a 32-edge half with
//     one K = 32 MFMA, whose k slots are the C layout of two edge blocks;
//   * a k1 chunk runs HALF-CHUNK-MAJOR: edge blocks {0, 1} over all eight column blocks (48 MFMAs), then edge blocks {2, 3}
//     (48 MFMAs); a half is four batches of two column blocks (fragments: two sets of 16 registers, the next batch's set
//     read during the current one - every fragment twice per chunk, 32 ds_read_b128, one per three MFMA gaps; the image
//     variant: four resident sets, every fragment once, last item below) x two edge
//     blocks x 6 MFMAs.  An MFMA of this shape leaves the SIMD's issue port free for about half of its 16 cycles, i.e. for
//     two vector instructions, so the K loop is LEVELLED: no gap of the steady chunk carries more than two vector / LDS /
//     DMA instructions (three where hipcc adds an address add).  The A operands are single-buffered: while a half runs,
//     the other half's 16 operand registers are free, and the next operands are converted into them ONE instruction per
//     gap (40 per half over 48 gaps; schedule at the loop);
//   * MFMA order is pinned by an empty asm on the accumulator ("+a") after every MFMA plus
//     sched_barrier(0): hipcc otherwise sinks the MFMAs of a step below its conversions;
//   * H1 is produced by asm MFMAs with a VGPR destination (the builtin lands in AGPRs in a 512-register
//     kernel: one v_accvgpr_read per value), in two halves of four per chunk, and converted by single-instruction asm
//     statements (relu, relu, rtz16 hi, rn16 lo low / high half) - hipcc pads no hazards for asm operands, so each producer
//     is placed >= 2 MFMAs before its first consumer, and a converted register is written a whole gap or more ahead of
//     the first MFMA that reads it;
//   * W2 chunk images (16 KiB, pre-swizzled) stream through a 3-slot LDS ring by LDS-DMA: chunk c + 2 is
//     issued during chunk c (4 pieces per wave, one address + immediate offsets, in gaps that carry nothing else), retired
//     by the s_waitcnt vmcnt(0) + s_barrier that ends chunk c; fragments are read a batch ahead, in place;
//   * the forward's aggregation runs on the attribute operand image where the workspace holds one (ASRC_IMAGE, at the
//     kernel's template): no per-tile prologue, the tile boundary lies inside the tile's last chunk (DESIGN.md §3d,
//     "The tile boundary");
//   * the image variant (209 VGPRs with two fragment sets) keeps FOUR RESIDENT sets, 64 registers: batch bt of either half
//     reads set bt, so every fragment is read from LDS once per chunk - 16 ds_read_b128, not 32.  Chunk c + 1's sets 0, 1, 2
//     are read from its ring slot during chunk c's second-half batches 1, 2, 3 (behind the set's last MFMA of chunk c, two
//     batches or more ahead of its first of chunk c + 1), its set 3 during its own second batch, two batches ahead; same
//     gaps (q = 0, 3, 6, 9), and three batches of the first half carry no fragment read.  The 3-slot ring allows it:
//     chunk c + 1's pieces were issued during chunk c - 1 and retired by the wait and barrier that closed it; during chunk
//     c only the slot of chunk c + 2 is written, which was the slot of chunk c - 1 - whose last fragment read (its set 3)
//     ran in front of that same barrier.  The sets do not live across the aggregation phase (g2hi / g2lo take their
//     registers): a tile reads set 0 up front, as before, and sets 1, 2, 3 in the first three batches of its chunk 0, a
//     batch ahead each; its last chunk reads nothing for a next chunk.  MFMA order and operands are those of the two-set
//     schedule, which the other four instantiations keep line for line ("Resident fragments");
//   * the image variant's product MFMAs are asm statements with a TIED accumulator (one "+a" operand is C and D; as builtins
//     hipcc rotated them through a[0:3] - `acc` and `Z` fill the AGPRs - and parked accumulators in VGPRs around the peeled
//     chunks' side loads).  A tile's first product into each accumulator (chunk 0, hi x lo) takes the inline constant 0 as C:
//     nothing zeroes `acc`.  hipcc pads no wait states around an asm MFMA, so: A operands are written a whole gap or more ahead
//     (conversion schedule), and the only non-MFMA reader of an accumulator, the un-scale, sits behind the last chunk's
//     barrier, 16 wait states and an opaque "+a" on every accumulator.  Same products, same order, same rounding (DESIGN.md
//     §3d, "Tied accumulators").
#include "gpde_common.h"
#include <cstdlib>
#include <type_traits>

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma32k(h8 a, h8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
#define GPDE_GLDS(g, l, off)                                                                       \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g),         \
                                     (__attribute__((address_space(3))) void*)(l), 16, off, 0)

__device__ __forceinline__ int lower_bound_node(const int32_t* __restrict__ rowptr, int lo, int hi, long target) {
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if ((long)rowptr[mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

#ifdef GPDE_V6_TIMING      // developer probe (scripts/v6_timing.py): cycles per phase summed over waves, wave-tiles
__device__ unsigned long long gpde_v6_tm[8];      // prologue, K loop, post, tiles, peeled chunks 0-5 (part of the K loop)
#define TM_MARK(acc) do { const long long tm1_ = clock64(); acc += tm1_ - tm0_; tm0_ = tm1_; } while (0)
#else
#define TM_MARK(acc) do { } while (0)
#endif

constexpr int NS = 3;                      // W2 ring slots
constexpr int TILE_B = GP_TN * 128;        // 16 KiB per W2 chunk image: [128 columns][hi 64 B | lo 64 B]
constexpr int TE = 64;                     // edges per wave tile (four MFMA row blocks of 16)
constexpr int NW = 4;                      // waves per workgroup

// WRITE_H: the store variant (gpde_hidden_fwd, the backward's recompute of H_2, the per-edge path of gpde_api.hip): the
// hidden activations of the tile go to a.hout ([CSR slot][K2P] fp32) instead of into the aggregation; no x_j, no Z, static
// edge ranges (rows are independent).
// NODEATTR (gpde_nnconv_fwd_nodeattr): the edge attributes are not a tensor - slot d of edge
// (j -> i) is table[(sel[d] >> 8 ? i : j) * kt + (sel[d] & 255)], read from the node table (a.attr) with the tile's
// source / destination ids (the reference builds the [E, 6] tensor from node data, utilities.py:274-277).  No `perm`,
// no per-edge attribute traffic: the table (N x kt floats) lives in L2.
// ASRC 2, the attribute operand IMAGE (aggregation variant only; gpde_launch_attr_image built it for this call): B1 and the
// per-edge un-scale are not formed per tile but fetched - the next tile's 64 rows of the hi plane, the lo plane and isc by
// three LDS-DMA in the tile's chunk 2, into a per-wave staging area and the other parity of a double-buffered `Es`.  The
// tile boundary moves into the tile's LAST chunk (peeled, PH 7): it reads the next tile's B1 from the staging area in its
// first gaps, its two H1 halves are the next tile's chunk-0 raw H1 (c1 wraps to the chunk-0 rows of (W1|b1)) and the
// conversions of its second half the next tile's operands of edge blocks {0, 1}.  What is left between two tiles is
// the round flags with their barrier and the first fragment reads; only a wave's first tile forms its operands up front.
enum { ASRC_TENSOR = 0, ASRC_NODES = 1, ASRC_IMAGE = 2 };
template <int MODE, int ASRC = ASRC_TENSOR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void gpde_fused_f16v6_kernel(GpdeFusedArgs a) {
    constexpr bool WRITE_H = MODE == 1;       // store variant
    constexpr bool NODEATTR = ASRC == ASRC_NODES, IMAGE = ASRC == ASRC_IMAGE;
    static_assert(!(IMAGE && WRITE_H), "the store variant forms its attribute operands itself");
    extern __shared__ __attribute__((aligned(16))) char smem[];     // ONE LDS object (cdna guide, glds trap a)
    char* ring = smem;                                               // [3][16 KiB]
    char* w1s = smem + NS * TILE_B;                                  // [K1P][hi 16 B | lo 16 B]
    unsigned* Xs_all = (unsigned*)(w1s + (size_t)a.K1P * 32);        // [4 waves][64 rows][64 words]
    float* Es_all = (float*)(Xs_all + NW * TE * GP_W);               // [4][64]
    int* red = (int*)(Es_all + NW * TE);                             // [2][4]
    float* colc = (float*)(red + 16);                                // [2][128]: scaled b2 | un-scale factor of the slice's columns

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15;                // MFMA row (A) / column (B, C, D) of this lane
    const int g = lane >> 4;                  // lane group: k slots 8g .. 8g+7 (A, B), rows 4g .. 4g+3 (C, D)
    float* Es = Es_all + wave * TE;
    unsigned* Xs = Xs_all + wave * TE * GP_W;
    // IMAGE: red[8..11] is a zeroed 16-byte slot (lane group 3's attribute operand); behind colc a staging area per wave
    // ([hi rows 1 KiB | lo rows 1 KiB] of the next tile's 64 edges) and the second parity of Es, [4][64].  `Es` is the
    // current tile's parity, Es_n the one the next tile's isc is fetched into; they swap per tile
    char* stage = nullptr;
    float* Es_n = nullptr;
    if constexpr (IMAGE) {
        stage = (char*)(colc + 2 * GP_TN) + wave * 2048;
        Es_n = (float*)((char*)(colc + 2 * GP_TN) + NW * 2048) + wave * TE;
    }

    const int ns = a.K2P / GP_TN;
    const int slice = blockIdx.x % ns;
    const int group = blockIdx.x / ns;
    const int NKC = a.K1P / GP_BK;

    for (int i = tid; i < a.K1P * 2; i += 256) ((f32x4*)w1s)[i] = ((const f32x4*)a.w1h)[i];

    // ---- work assignment ---------------------------------------------------------------------------------
    // Queue mode (a.blk != nullptr, the default): the chunk's edges are cut into node-aligned BLOCKS of ~4096 edges
    // (a.blk[b] .. a.blk[b+1], gpde_prep.hip) and every wave draws its next block from ONE counter per column slice
    // (a.qctr[slice]; the workgroups of a slice share an XCD).  The 128 waves of a slice therefore work on
    // CONSECUTIVE blocks at any time - a window of a few hundred destination nodes whose sources (x_j rows) are the
    // same lattice band for all of them, so the gather hits in the XCD's L2 (4 MiB) instead of missing it on every
    // edge (measured: HBM-side fetch per launch 56 GB with contiguous per-wave ranges).  A node's in-edges lie in one
    // block and one wave walks them in CSR order: the sum order does not depend on which wave drew the block -
    // results stay bit-reproducible.  The queue also levels the load (the tail is one block, not one range).
    // Static mode (a.blk == nullptr): one contiguous node-aligned range per wave.
    const int e_lo = a.rowptr[a.nc0], e_hi = a.rowptr[a.nc1];
    const bool queue = a.blk != nullptr;
    int blk_a = 0, blk_b = 0;           // current block / range [blk_a, blk_b)
    const int nblk = queue ? *a.qn : 0;
    bool have;
    auto draw_block = [&](int& ba, int& bb) {        // wave-uniform; false when the queue is empty
        for (;;) {
            int b = 0;
            if (lane == 0) b = (int)atomicAdd(a.qctr + slice, 1u);
            b = __builtin_amdgcn_readfirstlane(b);
            if (b >= nblk) return false;
            ba = a.blk[b];
            bb = a.blk[b + 1];
            if (bb > ba) return true;
        }
    };
    if (queue) {
        have = draw_block(blk_a, blk_b);
    } else {
        const long tot = (long)e_hi - e_lo;
        const int nranges = a.n_groups * NW;
        const int wg = group * NW + wave;
        const int na = lower_bound_node(a.rowptr, a.nc0, a.nc1, e_lo + tot * wg / nranges);
        const int nb_ = (wg == nranges - 1) ? a.nc1
                                            : lower_bound_node(a.rowptr, a.nc0, a.nc1, e_lo + tot * (wg + 1) / nranges);
        blk_a = a.rowptr[na];
        blk_b = a.rowptr[nb_];
        have = blk_b > blk_a;
    }
    // red[parity][wave]: "this wave has no tile" flags of the current tile round (double-buffered by parity)
    if (lane == 0) { red[wave] = have ? 0 : 1; red[4 + wave] = 0; }
    if constexpr (IMAGE) {
        if (tid < 4) red[8 + tid] = 0;
    }
    __syncthreads();
    if (red[0] + red[1] + red[2] + red[3] == 4) return;

    // ---- W2 chunk DMA: 4 x 1 KiB per wave per chunk, one address, immediate offsets on both sides -----
    const unsigned long long w2base = (unsigned long long)a.w2h + (size_t)slice * NKC * TILE_B + wave * 4096;
    const unsigned lane16 = lane * 16;
    auto w2_src = [&](int chunk) {
        unsigned long long gb = w2base + (size_t)chunk * TILE_B;
        asm volatile("" : "+s"(gb));
        return (const char*)(gb + lane16);
    };

    // constants of the un-scaling: h <= max|b2| + max_k ||W2_k||_1 * max_e B_e (pack-time constants in fcol[8..9])
    // (per column, read back per column block after the K loop: 16 registers would not fit beside the K loop's)
    float z_unscale = 1.f;
    if constexpr (WRITE_H) {
        if (tid < GP_TN) {
            colc[tid] = a.b2[slice * GP_TN + tid];
            colc[GP_TN + tid] = a.ucol[slice * GP_TN + tid];
        }
    } else {
        const float sx = gpde_pow2_to_2p13(__uint_as_float(a.scal[0]));
        const float hb = a.fcol[8] + a.fcol[9] * __uint_as_float(a.scal[1]);
        const float sh = gpde_pow2_to_2p13(hb);
        if (tid < GP_TN) {
            colc[tid] = a.b2[slice * GP_TN + tid] * sh;                  // exact: sh is a power of two
            colc[GP_TN + tid] = a.ucol[slice * GP_TN + tid] * sh;
        }
        z_unscale = (1.f / sx) * (1.f / sh);      // two exact reciprocals: sx * sh may exceed the float range
    }
    float wmx8[8], fcol8[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        wmx8[d] = a.w1[(size_t)a.K1P * 8 + (d & 1) * 4 + (d >> 1)];
        fcol8[d] = a.fcol[d];
    }
    // W2 fragment of column 16 nb + l15: chunk-image row = column (128 B: units 0-3 hi, 4-7 lo; unit u = 2m + h holds, at
    // position j, k = 16m + 8 (j >> 2) + 4h + (j & 3) of the chunk - gpde_pack.hip), unit position swizzled by
    // (column >> 1) & 7; lane group g reads unit g (hi) and 4 + g (lo = position ^ 64).  A column block is 16 rows = 2 KiB.
    // Within 16 lanes the sixteen 16-byte positions are distinct (8 (c & 1) + (c >> 1) mod 16)
    const int bo = l15 * 128 + ((g ^ ((l15 >> 1) & 7)) << 4);
    // (W1|b1) row of H1 row l15 in the chunk's first 16-row half (second half: 8 rows = 256 B on).  D row i = 4g' + r of
    // half hf comes from W1 row k(g', 4 hf + r) = 16 (g' >> 1) + 8 hf + 4 (g' & 1) + r, so that after both halves lane
    // group g holds, at position j = 4 hf + r, exactly the k of unit g's position j - the A operand of the hidden-layer
    // MFMA without a cross-lane move.  Lane groups 0, 1 read the row's hi 16 bytes, 2 its lo 16 bytes, 3 the hi again
    // (finite; its attribute operand is zero)
    const int w1o = (16 * (l15 >> 3) + 4 * ((l15 >> 2) & 1) + (l15 & 3)) * 32 + (g == 2 ? 16 : 0);

    // ---- per-tile side loads ----------------------------------------------------------------------------
    const int e_clamp = max(e_hi - 1, 0);
    // lane l owns edge (tile start + l): its edge id, source node and 8 attribute slots; the MFMA operand
    // layout needs edge 16 b + (l & 15) in ALL FOUR lane groups - broadcast by ds_bpermute in the prologue
    int perm_n = 0;
    [[maybe_unused]] int dst_n = 0;     // NODEATTR: perm_n holds the SOURCE node of the next tile's edge, dst_n its destination
    int src_l = 0;                      // source node of edge (tile start + lane), for the x_j row DMA
    float attr_n[8];
    auto load_perm = [&](int e0n) {
        if constexpr (NODEATTR) {
            perm_n = a.src[min(e0n + lane, e_clamp)];
            dst_n = a.dst[min(e0n + lane, e_clamp)];
        } else perm_n = a.perm[min(e0n + lane, e_clamp)];
    };
    auto load_attr_d = [&](int d) {             // one attribute slot (the K loop issues them one per MFMA gap)
        if constexpr (NODEATTR) {
            const int sd = a.sel[d];                                         // scalar (kernel argument)
            attr_n[d] = a.attr[(size_t)((sd >> 8) ? dst_n : perm_n) * a.kt + (sd & 255)];
        } else {
            attr_n[d] = a.attr[(size_t)perm_n * a.k0 + min(d, a.k0 - 1)];
        }
    };
    auto load_attr = [&]() {
#pragma unroll
        for (int d = 0; d < 8; ++d) load_attr_d(d);
    };
    // IMAGE: the three LDS-DMA of a tile that starts at CSR slot e0t in a block that ends at ebt (0: no tile) - lane l
    // fetches edge e0t + l's row of the hi plane, of the lo plane (16 bytes each, to the staging area) and its isc (4 bytes,
    // to `es_to`).  A lane without an edge fetches the constant record (zeros | 1.0f): masking is one address select, and
    // no lane reads past the image
    [[maybe_unused]] auto img_issue = [&](int which, int e0t, int ebt, float* es_to) {
        const int e = e0t + lane;
        const bool ok = e < ebt;
        if (which == 0) {
            const char* p = ok ? (const char*)a.img_hi + (size_t)e * 16 : (const char*)a.img_rec;
            GPDE_GLDS(p, stage, 0);
        } else if (which == 1) {
            const char* p = ok ? (const char*)a.img_lo + (size_t)e * 16 : (const char*)a.img_rec;
            GPDE_GLDS(p, stage + 1024, 0);      // (an immediate offset would move the global side too)
        } else {
            const char* p = ok ? (const char*)(a.img_isc + e) : (const char*)a.img_rec + 16;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)p,
                                             (__attribute__((address_space(3))) void*)es_to, 4, 0, 0);
        }
    };
    // where lane (l15, g) reads B1 of edge block b from the staging area: block 0's address and the stride per block -
    // lane group 1 the lo rows, groups 0 and 2 the hi rows, group 3 the zeroed slot (stride 0)
    const char* b1p = nullptr;
    int b1s = 0;
    if constexpr (IMAGE) {
        b1p = g == 3 ? (const char*)(red + 8) : stage + l15 * 16 + (g == 1 ? 1024 : 0);
        b1s = g == 3 ? 0 : 256;
    }
    // x_j rows of this tile: piece i = rows 4i .. 4i+3 (lane >> 4 picks the row, lane & 15 its 16-byte unit).
    // The source node comes from the lane that loaded that edge's src (ds_bpermute) at the START of a chunk,
    // the four DMA are issued at its END, behind the chunk's W2 pieces (see the K loop).
    int xsidx[4];
    auto x_addr1 = [&](int i0, int i) { xsidx[i] = __builtin_amdgcn_ds_bpermute((4 * (i0 + i) + (lane >> 4)) * 4, src_l); };
    auto x_issue1 = [&](int i0, int i) {
        int unit = lane & 15;
        GPDE_GLDS(a.xs + (size_t)xsidx[i] * GP_W + unit * 4, Xs + (i0 + i) * 4 * GP_W, 0);
    };

    // ---- conversions and H1 generation (asm: see the header) ----------------------------------------------
    auto conv_a = [&](float v0, float v1, unsigned& ph, unsigned& t0_, unsigned& t1_) {
        asm("v_max_i32 %1, 0, %3\n\t"
            "v_max_i32 %2, 0, %4\n\t"
            "v_cvt_pkrtz_f16_f32 %0, %1, %2"
            : "=&v"(ph), "=&v"(t0_), "=&v"(t1_) : "v"(v0), "v"(v1));
    };
    auto conv_b = [&](unsigned ph, unsigned t0_, unsigned t1_, unsigned& pl) {
        asm("v_fma_mixlo_f16 %0, %1, 1.0, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixhi_f16 %0, %2, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
            : "=&v"(pl) : "v"(t0_), "v"(t1_), "v"(ph));
    };
    auto conv_pair = [&](float v0, float v1, unsigned& ph, unsigned& pl) {      // both parts (outside the K loop)
        unsigned t0_, t1_;
        conv_a(v0, v1, ph, t0_, t1_);
        conv_b(ph, t0_, t1_, pl);
    };
    // One conversion instruction (step 0..4 of a pair: relu, relu, hi = rtz16, lo = rn16(y - hi) low / high half), as a statement
    // of its own: the K loop issues ONE per MFMA gap.  The same five instructions as conv_a + conv_b
    auto conv_step = [&](int step, float v0, float v1, unsigned& ph, unsigned& t0_, unsigned& t1_, unsigned& pl) {
        if (step == 0) asm("v_max_i32 %0, 0, %1" : "=v"(t0_) : "v"(v0));
        if (step == 1) asm("v_max_i32 %0, 0, %1" : "=v"(t1_) : "v"(v1));
        if (step == 2) asm("v_cvt_pkrtz_f16_f32 %0, %1, %2" : "=v"(ph) : "v"(t0_), "v"(t1_));
        if (step == 3) asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(pl) : "v"(t0_), "v"(ph));
        if (step == 4) asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(pl) : "v"(t1_), "v"(ph));
    };
    // ONE MFMA per 16 H1 rows x 16 edges: K = 32 holds the three split terms, by lane group W1hi x attr_hi |
    // W1hi x attr_lo | W1lo x attr_hi | (anything) x 0.  The leading s_nop covers a VALU write of an operand right in
    // front of the statement
    auto h1gen_half = [&](f32x4 (&dd)[4][2], int e0, h8 w1r0, h8 w1r1, const h8 (&at)[4]) {      // edge blocks e0, e0 + 1: 4 MFMAs
        asm volatile("s_nop 4");
#pragma unroll
        for (int e = e0; e < e0 + 2; ++e) {
            asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(dd[e][0]) : "v"(w1r0), "v"(at[e]));
            asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(dd[e][1]) : "v"(w1r1), "v"(at[e]));
        }
    };
    // Product MFMA of the hidden layer with a TIED accumulator (image variant): one "+a" operand is C and D, so hipcc cannot
    // rotate the accumulators through spare registers or park them in VGPRs.  An accumulate chain into the same D needs no
    // wait states; the A operand comes from conversions a whole gap or more ahead (K-loop schedule), the B operand from
    // ds_read_b128 that hipcc still waits for.  Any OTHER reader of the accumulator needs the MFMA's wait states first -
    // see the end of the K loop
    // `first`: an accumulator's first product of a tile (chunk 0, hi x lo) takes the inline constant 0 as C and writes the
    // accumulator as a plain output - nothing zeroes `acc`, and nothing a tile (or a round without a tile) left in it is
    // added to.  `pad`: two wait states in front (a VALU write of the A operand at no fixed distance)
    [[maybe_unused]] auto prod_tied = [&](f32x4& c, u4 av, h8 bv, bool first, bool pad) {
        if (first && pad) asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=a"(c) : "v"(av), "v"(bv));
        else if (first) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=a"(c) : "v"(av), "v"(bv));
        else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(av), "v"(bv));
    };
    auto h1gen = [&](f32x4 (&dd)[4][2], h8 w1r0, h8 w1r1, const h8 (&at)[4]) {      // the 8 MFMAs of a chunk (tile prologue)
        h1gen_half(dd, 0, w1r0, w1r1, at);
        h1gen_half(dd, 2, w1r0, w1r1, at);
    };

    // ---- prologue: chunks 0 and 1 of the W2 slice, the first tile's edges and attributes ---------------
    {
        const char* g0 = w2_src(0);
        char* l0 = ring + wave * 4096;
        GPDE_GLDS(g0, l0, 0); GPDE_GLDS(g0, l0, 1024); GPDE_GLDS(g0, l0, 2048); GPDE_GLDS(g0, l0, 3072);
        const char* g1 = w2_src(1);
        char* l1 = ring + TILE_B + wave * 4096;
        GPDE_GLDS(g1, l1, 0); GPDE_GLDS(g1, l1, 1024); GPDE_GLDS(g1, l1, 2048); GPDE_GLDS(g1, l1, 3072);
    }
    if constexpr (IMAGE) {
#pragma unroll
        for (int i = 0; i < 3; ++i) img_issue(i, have ? blk_a : e_hi, have ? blk_b : 0, Es);
    } else {
        load_perm(have ? blk_a : e_hi);
        load_attr();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // acc[edge block][column block]: edge 16 e + 4g + r, column 16 nb + l15;  Z[channel block][column block]: channel
    // 16 cb + 4g + r, column 16 nb + l15
    f32x4 acc[4][8], Z[4][8];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int nb = 0; nb < 8; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (!IMAGE) acc[e][nb][r] = 0.f;      // (IMAGE: chunk 0's first products take C = 0)
                Z[e][nb][r] = 0.f;
            }
    int cur = -1;
    [[maybe_unused]] float hmax_run = 0.f;      // WRITE_H: running maximum of the stored activations (>= 0)

    // one plain-store flush per (node, slice): the row base is wave-uniform (scalar address arithmetic), the lane
    // part of the address is ONE offset - 16 per-row vector addresses would be hoisted out of the tile loop and spilled
    auto flush = [&](int node) {
        float* zb = a.zbuf + ((size_t)(node - a.nc0) * GP_W) * a.K2P + slice * GP_TN;
        int zl = lane;
        asm volatile("" : "+v"(zl));            // opaque: the lane offset is computed here (a few VALU per node), not kept
        const int z_loff = 4 * (zl >> 4) * a.K2P + (zl & 15);       // across the tile loop in two more registers
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int nb = 0; nb < 8; ++nb) asm volatile("" : "+a"(Z[cb][nb]));
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float* rp = zb + (size_t)(cb * 16 + r) * a.K2P;
#pragma unroll
                for (int nb = 0; nb < 8; ++nb) {
                    rp[z_loff + nb * 16] = Z[cb][nb][r] * z_unscale;      // 64-byte runs (16 lanes x 4 B)
                    Z[cb][nb][r] = 0.f;
                }
                if ((r & 1) == 1) __builtin_amdgcn_sched_barrier(0);      // 16 values in flight, not 128
            }
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int nb = 0; nb < 8; ++nb) asm volatile("" : "+a"(Z[cb][nb]));
    };

    int slot = 0;           // ring slot of the current chunk

#ifdef GPDE_V6_TIMING
    long long tm_pro = 0, tm_loop = 0, tm_post = 0, tm_peel = 0, tm0_ = clock64();
#endif
    int e0 = have ? blk_a : e_hi;
    int n_rounds = 0;
    // B1[e]: H1 MFMA operand per edge block, by lane group: attr_hi | attr_lo | attr_hi | 0
    // d[e][half][r]: H1 of edge 16 e + l15, operand position j = 4 half + r of lane group g;  ahi / alo[e]: j = 0..7 as f16 pairs
    // (IMAGE: B1, d[2..3] and ahi / alo[0..1] are carried from a tile's last chunk into the next tile)
    h8 B1[4];
    f32x4 d[4][2];
    u4 ahi[4], alo[4];                // single-buffered: see the conversion schedule in the K loop
    if constexpr (IMAGE) {
        // cold start, once per wave and launch: the first tile's operands from the staging area, raw H1 of chunk 0, the
        // operands of edge blocks {0, 1} (chunk 0 converts {2, 3} in its first half)
#pragma unroll
        for (int b = 0; b < 4; ++b) B1[b] = *(const h8*)(b1p + b * b1s);
        const char* wp = w1s + w1o;
        const h8 A1 = *(const h8*)wp, A2 = *(const h8*)(wp + 256);
        h1gen(d, A1, A2, B1);
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");           // MFMA result -> VALU read (asm operands are not padded)
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int jp = 0; jp < 4; ++jp) {
                unsigned ph, pl;
                conv_pair(d[e][jp >> 1][2 * (jp & 1)], d[e][jp >> 1][2 * (jp & 1) + 1], ph, pl);
                ahi[e][jp] = ph;
                alo[e][jp] = pl;
            }
    }
    for (int t = 0;; ++t) {
        // ---- this tile, and where the NEXT one starts (its edge ids / attributes are prefetched during this one) ----
        const int eb = have ? blk_b : e0;                        // no tile: everything below is masked out
        const int e_end = min(e0 + TE, eb);
        const bool last_in_blk = have && (e0 + TE >= blk_b);
        int na_ = 0, nb_ = 0;
        bool have_n = have && !last_in_blk;
        if (last_in_blk && queue) have_n = draw_block(na_, nb_);      // drawn ONE tile ahead: no block is held in reserve
        const int e0n = !have ? e_hi : (last_in_blk ? (have_n ? na_ : e_hi) : e0 + TE);
        [[maybe_unused]] const int ebn = !have ? 0 : (last_in_blk ? (have_n ? nb_ : 0) : blk_b);     // its block's end (0: no next tile)
        if (t > 0) {
            // all four waves out of tiles -> done.  Flags of this round were written before the barrier; the other
            // parity is rewritten two rounds later, behind at least one K loop of barriers
            if (lane == 0) red[(t & 1) * 4 + wave] = have ? 0 : 1;
            __syncthreads();
            const int* rf = red + (t & 1) * 4;
            if (rf[0] + rf[1] + rf[2] + rf[3] == 4) break;
        }
        ++n_rounds;

        // ---- attributes of this lane's two edges: validity, bias slot, per-edge scale, f16 split ------------
        // (IMAGE: the tile's last chunk read them from the staging area, its isc is in Es)
        if constexpr (!IMAGE) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                float av[8];    // attributes of edge 16 b + l15, in all four lane groups
#pragma unroll
                for (int d = 0; d < 8; ++d)
                    av[d] = __int_as_float(__builtin_amdgcn_ds_bpermute((16 * b + l15) * 4, __float_as_int(attr_n[d])));
                const bool valid = (e0 + 16 * b + l15) < eb;
                float v[8];
                float bnd = 0.f;
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    float q = (valid && d < a.k0) ? av[d] : 0.f;
                    if (valid && d == a.k0) q = 1.f;
                    v[d] = q;
                    bnd = fmaf(wmx8[d], fabsf(q), bnd);
                }
                const int ebits = (__float_as_int(bnd) >> 23) & 0xff;
                const bool okb = (ebits >= 20) && (ebits <= 230);
                const float sc = okb ? __int_as_float((267 - ebits) << 23) : 1.f;     // 2^(13 - E(B))
                const float isc = okb ? __int_as_float((ebits - 13) << 23) : 1.f;
                if (g == 0) Es[16 * b + l15] = isc;
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    const float s_ = v[d] * fcol8[d] * sc;
                    const _Float16 hi = (_Float16)s_;
                    const _Float16 lo = (_Float16)(s_ - (float)hi);
                    B1[b][d] = g == 1 ? lo : (g == 3 ? (_Float16)0.f : hi);
                }
            }
        }
        // W2 fragments of the chunk's first batch (column blocks 0, 1).  A chunk is four batches of two column blocks;
        // the 32 fragment registers are two sets, the next batch's set is read during the current batch (not carried
        // across the aggregation phase)
        // IMAGE: FOUR sets, one per batch of a half and resident for the chunk (see the header); chunk 0 reads sets 1-3 in its
        // own first gaps
        constexpr int NFS = IMAGE ? 4 : 2;
        h8 bhi[NFS][2], blo[NFS][2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            bhi[0][nb] = *(const h8*)(ring + slot * TILE_B + nb * 2048 + bo);
            blo[0][nb] = *(const h8*)(ring + slot * TILE_B + nb * 2048 + (bo ^ 64));
        }
        // ---- raw H1 of chunk 0 and the operands of chunk 0 -----------------------------------------------
        // (IMAGE: the last chunk of the tile before produced them, or the cold start)
        if constexpr (!IMAGE) {
            const char* wp = w1s + w1o;
            const h8 A1 = *(const h8*)wp, A2 = *(const h8*)(wp + 256);
            h1gen(d, A1, A2, B1);
            asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");           // MFMA result -> VALU read (asm operands are not padded)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int jp = 0; jp < 4; ++jp) {
                    unsigned ph, pl;
                    conv_pair(d[e][jp >> 1][2 * (jp & 1)], d[e][jp >> 1][2 * (jp & 1) + 1], ph, pl);
                    ahi[e][jp] = ph;
                    alo[e][jp] = pl;
                }
        }
        // destination of the first / last edge of the two 32-edge halves: loaded with the other side loads at the
        // end of chunk 0 (all lanes the same address), made scalar after the K loop
        int nf_v[2] = {0, 0}, nl_v[2] = {0, 0};
        unsigned cph = 0, ct0 = 0, ct1 = 0, cpl = 0;
        h8 A1, A2;

        // One k1 chunk.  The first seven chunks of a tile are peeled (PH = compile-time phase) so that the side
        // loads are straight-line code: inside a runtime `if (c == ..)` hipcc copies the loaded registers into
        // their loop-carried homes and waits vmcnt(0) for them right behind the load (measured: one exposed
        // memory round trip per chunk, ~40 % of the tile).  Side loads are issued at the END of a chunk, BEHIND
        // its four W2 pieces, and the closing wait is vmcnt(<side loads of this chunk>): the W2 pieces are
        // retired, the side loads fly for a whole chunk and are retired by the next chunk's closing wait.
        //   PH 0: next tile's edge ids, this tile's source nodes, 4 segment-end nodes (6 loads)   -> vmcnt(6)
        //         (NODEATTR: next tile's source AND destination ids instead of the edge ids: 7 loads -> vmcnt(7))
        //   PH 1: nothing (the three loads land)                                                   -> vmcnt(0)
        //   PH 2: next tile's attributes (8 loads) + x_j rows 0..15 (4 DMA)                        -> vmcnt(12)
        //   PH 3/4/5: x_j rows 16..31 / 32..47 / 48..63 (4 DMA each)                               -> vmcnt(4)
        //   PH 6: steady state                                                                     -> vmcnt(0)
        // IMAGE (no edge ids, no attribute loads; the tile's LAST chunk is peeled too):
        //   PH 0: this tile's source nodes, 4 segment-end nodes (5 loads)                          -> vmcnt(5)
        //   PH 1: nothing                                                                          -> vmcnt(0)
        //   PH 2: next tile's hi rows, lo rows, isc (3 DMA) + x_j rows 0..15 (4 DMA)               -> vmcnt(7)
        //   PH 3/4/5, PH 6: as above (PH 3's wait retires the three image DMA)                     -> vmcnt(4), vmcnt(0)
        //   PH 7: the last chunk: next tile's B1 from the staging area, its chunk-0 raw H1 and operands {0, 1} -> vmcnt(0)
        TM_MARK(tm_pro);
        auto chunk = [&](auto ph_tag, int c) {
            constexpr int PH = decltype(ph_tag)::value;
            asm volatile("" : "+s"(c));         // opaque: keeps the peeled chunks' addresses from being hoisted out of
                                                // the tile loop (and spilled)
            const int slot1 = slot + 1 == NS ? 0 : slot + 1;
            const int slot2 = slot1 + 1 == NS ? 0 : slot1 + 1;
            int c2 = c + 2;
            if (c2 >= NKC) c2 -= NKC;
            const char* gsrc = w2_src(c2);
            char* ldst = ring + slot2 * TILE_B + wave * 4096;
            const char* rb0 = ring + slot * TILE_B;
            const char* rb1 = ring + slot1 * TILE_B;
            int c1 = c + 1;                                               // (W1|b1) rows read in this chunk: chunk c + 1
            if (c1 >= NKC) c1 -= NKC;
            const char* w1n = w1s + (size_t)c1 * GP_BK * 32 + w1o;
            // 96 MFMAs in HALF-CHUNK-MAJOR order: edge blocks {0, 1} over all eight column blocks (n = 0..47), then edge blocks
            // {2, 3} (n = 48..95).  A half is four batches of two column blocks, a batch 12 MFMAs: edge block 2 hf, then 2 hf + 1,
            // six each (three split products x two column blocks, product-major so that consecutive MFMAs go to different
            // accumulators; every accumulator still receives hi x lo, hi x hi, lo x hi of a chunk in that order).  The fragment
            // set alternates per batch (g8 & 1: eight batches, so the sets line up from chunk to chunk), and a batch's fragments
            // are read during the batch before it - twice per chunk, since both halves need all eight column blocks.
            // n = MFMA index in the chunk, q = n % 12 its index in the batch; what rides in the gap behind MFMA n - at most TWO
            // vector / LDS / DMA instructions in the steady chunk, because an MFMA of this shape leaves the SIMD's issue port
            // free for about 8 of its 16 cycles ("The levelled K loop"):
            //   conversions   a half never reads the OTHER half's operand registers (single buffer), so they are converted
            //                 there: this chunk's edge blocks {2, 3} in n = 0..46, the next chunk's {0, 1} in n = 48..94.
            //                 ONE instruction per gap (conv_step: relu, relu, hi, lo-low, lo-high of a pair), batch bt does
            //                 pairs 2 bt, 2 bt + 1 of the half's eight in q = 0..4 and 6..10; q = 5 and 11 carry none.
            //                 A converted register is written at least a whole gap ahead of its first MFMA reader (n = 46
            //                 before n = 54; n = 94 before the next chunk's n = 6), so no hazard pad is needed between them.
            //                 At a tile's first chunk the first half re-converts chunk 0's edge blocks {2, 3} from the unchanged
            //                 raw H1 (same values); at its last the second half converts the unused H1 below
            //   fragments     q = 0, 3, 6, 9: the next batch's four reads (lo 0, lo 1, hi 0, hi 1), into the other set
            //                 (IMAGE: the four reads of ONE resident set in four of the eight batches, see the batch loop)
            //   W2 ring       the four pieces at n = 5, 11, 17, 23
            //   (W1|b1)       n = 25, 31 (rows of chunk c + 1)
            //   raw H1        of chunk c + 1 in two halves of four MFMAs: edge blocks {0, 1} behind n = 45, {2, 3} behind
            //                 n = 93 - each behind the last conversion that read these registers (n = 94 of the chunk before,
            //                 n = 46) and two product MFMAs ahead of the first that reads the new values (n = 48, n = 0)
            //   side loads    peeled chunks only, in the conversion-free gaps n = 6 k + 5 behind the four W2 pieces (n >= 29), so
            //                 that the counted wait at the chunk end retires exactly the pieces; the ds_bpermute of the x_j
            //                 row addresses at n = 1, 7, 13, 19
#pragma unroll
            for (int g8 = 0; g8 < 8; ++g8) {
                const int hf = g8 >> 2, bt = g8 & 3, fs = IMAGE ? bt : (g8 & 1);      // half, batch of the half, fragment set
                // where the NEXT batch's fragments live: the next column blocks of this chunk (0, 1 again behind the first
                // half), behind the last batch 0, 1 of the next chunk; they go into set rs = the other one
                int rs = fs ^ 1;
                const char* rn = (g8 < 7) ? rb0 + (2 * ((bt + 1) & 3)) * 2048 : rb1;
                if constexpr (IMAGE) {
                    // resident sets: batch bt reads set bt in both halves, so this batch's gaps carry the reads of at most ONE
                    // set rs (none: rs < 0), each fragment once per chunk -
                    //   second half, bt = 1, 2, 3: set bt - 1 of chunk c + 1 from its slot (rb1), behind the set's last MFMA of
                    //     this chunk (batch bt - 1 of this half) and 2 batches or more ahead of its first of the next;
                    //   first half, bt = 1: set 3 of THIS chunk (its last MFMA ran in the chunk before), two batches ahead
                    //     (read in batch 0 or 2 instead, hipcc's peeled chunks carry 8 / 32 more accumulator copies);
                    //   a tile's chunk 0 (the sets do not live across the aggregation phase; set 0 was read at the tile start):
                    //     sets 1, 2, 3 in the first half's batches 0, 1, 2, a batch ahead each;
                    //   a tile's last chunk: nothing for a next chunk
                    rs = -1;
                    if (PH == 0 && hf == 0 && bt < 3) { rs = bt + 1; rn = rb0 + (2 * (bt + 1)) * 2048; }
                    else if (PH != 0 && g8 == 1) { rs = 3; rn = rb0 + 6 * 2048; }
                    else if (PH != 7 && hf == 1 && bt >= 1) { rs = bt - 1; rn = rb1 + (2 * (bt - 1)) * 2048; }
                }
#pragma unroll
                for (int q = 0; q < 12; ++q) {
                    const int e = 2 * hf + q / 6, j = q % 6;
                    const int tt = j >> 1, nb = j & 1;                    // tt: 0 = hi x lo, 1 = hi x hi, 2 = lo x hi
                    const int cb = 2 * bt + nb;
                    const int n = g8 * 12 + q;
#ifdef GPDE_ABL_2MFMA      // ablation build ONLY (scripts/gpu/clock_evidence.sh; WRONG results): two of the three split products, to
                           // measure how time and clock answer to a third less matrix work per edge
                    if (tt != 2)
#endif
                    if constexpr (IMAGE) {
                        // tied accumulator (header, last item): D = C by construction, C = 0 in a tile's first product of
                        // each accumulator.  A wave's first product follows the cold start's conversions of its A operand
                        // at no fixed distance: two wait states in the string
                        prod_tied(acc[e][cb], tt == 2 ? alo[e] : ahi[e], tt == 0 ? blo[fs][nb] : bhi[fs][nb],
                                  PH == 0 && tt == 0, PH == 0 && n == 0);
                    } else {
                        acc[e][cb] = mfma32k(__builtin_bit_cast(h8, tt == 2 ? alo[e] : ahi[e]),
                                             tt == 0 ? blo[fs][nb] : bhi[fs][nb], acc[e][cb]);
                        asm volatile("" : "+a"(acc[e][cb]));
                    }
                    if (q != 5 && q != 11) {
                        const int v = q < 5 ? q : q - 1, pr = 2 * bt + v / 5, step = v % 5;
                        const int ce = 2 * (1 - hf) + (pr >> 2), jp = pr & 3;
                        conv_step(step, d[ce][jp >> 1][2 * (jp & 1)], d[ce][jp >> 1][2 * (jp & 1) + 1], cph, ct0, ct1, cpl);
                        if (step == 4) {
                            ahi[ce][jp] = cph;
                            alo[ce][jp] = cpl;
                        }
                    } else {
                        // pins the pairs converted so far in their operand registers.  NOT in the gap of a pair's last
                        // instruction: hipcc pads an s_nop between that write and an asm statement reading it
                        const int ce = 2 * (1 - hf) + (bt >> 1);
                        asm volatile("" ::"v"(ahi[ce]), "v"(alo[ce]));
                    }
                    if (rs >= 0) {
                        if (q == 0) blo[rs][0] = *(const h8*)(rn + (bo ^ 64));
                        if (q == 3) blo[rs][1] = *(const h8*)(rn + 2048 + (bo ^ 64));
                        if (q == 6) bhi[rs][0] = *(const h8*)(rn + bo);
                        if (q == 9) bhi[rs][1] = *(const h8*)(rn + 2048 + bo);
                    }
                    if (n == 5) GPDE_GLDS(gsrc, ldst, 0);
                    if (n == 11) GPDE_GLDS(gsrc, ldst, 1024);
                    if (n == 17) GPDE_GLDS(gsrc, ldst, 2048);
                    if (n == 23) GPDE_GLDS(gsrc, ldst, 3072);
                    if (n == 25) A1 = *(const h8*)w1n;
                    if (n == 31) A2 = *(const h8*)(w1n + 256);
                    // The tile's side loads, ONE PER conversion-free gap behind the chunk's four W2 pieces, so that the counted
                    // wait at the chunk end retires exactly those (round 3: issued as one block after the last MFMA they cost
                    // ~570 cycles in each of the six peeled chunks, the matrix pipe idling while ~60 address / load
                    // instructions went out).  The x_j row addresses (ds_bpermute of the source ids loaded two chunks earlier)
                    // go into gaps of the first half.
                    if constexpr (MODE == 0 && PH == 0) {
                        if constexpr (!IMAGE) {
                            if (n == 53) load_perm(e0n);
                        }
                        if (n == 59) src_l = a.src[min(e0 + lane, e_clamp)];
                        if (n == 65) nf_v[0] = a.dst[min(e0, e_clamp)];
                        if (n == 71) nl_v[0] = a.dst[min(max(min(e0 + 32, eb) - 1, e0), e_clamp)];
                        if (n == 77) nf_v[1] = a.dst[min(e0 + 32, e_clamp)];
                        if (n == 83) nl_v[1] = a.dst[min(max(min(e0 + 64, eb) - 1, e0 + 32), e_clamp)];
                    } else if constexpr (WRITE_H && PH == 0) {
                        if (n == 53) load_perm(e0n);
                    }
                    if constexpr (PH == 2 && IMAGE) {
                        if (n == 29 || n == 35 || n == 41) img_issue((n - 29) / 6, e0n, ebn, Es_n);
                    } else if constexpr (PH == 2) {
                        if (n >= 29 && n < 77 && (n - 29) % 6 == 0) load_attr_d((n - 29) / 6);
                    }
                    if constexpr (PH == 7) {
                        // the next tile's B1: this tile's last reader of B1 was the H1 half behind n = 93 of the chunk before;
                        // gaps that carry one conversion and nothing else
                        if (n == 1) B1[0] = *(const h8*)b1p;
                        if (n == 2) B1[1] = *(const h8*)(b1p + b1s);
                        if (n == 4) B1[2] = *(const h8*)(b1p + 2 * b1s);
                        if (n == 7) B1[3] = *(const h8*)(b1p + 3 * b1s);
                    }
                    if constexpr (!WRITE_H && PH >= 2 && PH <= 5) {
                        if (n == 1 || n == 7 || n == 13 || n == 19) x_addr1(4 * (PH - 2), (n - 1) / 6);
                        if constexpr (PH == 2) {
                            if (n == 77 || n == 83 || n == 89 || n == 95) x_issue1(0, (n - 77) / 6);
                        } else {
                            if (n == 53 || n == 65 || n == 77 || n == 89) x_issue1(4 * (PH - 2), (n - 53) / 12);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (n == 45 || n == 93) {
                        // raw H1 of chunk c + 1, edge blocks {0, 1} / {2, 3}; at the last chunk this is chunk 0 with THIS
                        // tile's attributes - unused, the next tile starts afresh (IMAGE, PH 7: with the NEXT tile's
                        // attributes - the next tile's chunk-0 raw H1)
                        h1gen_half(d, n == 45 ? 0 : 2, A1, A2, B1);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            // closing wait: the chunk's W2 pieces are retired, its side loads (issued behind them, above) stay in flight
            if constexpr (WRITE_H && PH == 0 && NODEATTR) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");     // source + destination ids
            else if constexpr (WRITE_H && PH == 0) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
            else if constexpr (WRITE_H && PH == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else if constexpr (WRITE_H) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if constexpr (PH == 0 && NODEATTR) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
            else if constexpr (PH == 0 && IMAGE) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
            else if constexpr (PH == 0) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else if constexpr (PH == 2 && IMAGE) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
            else if constexpr (PH == 2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
            else if constexpr (PH >= 3 && PH <= 5) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            slot = slot1;
        };
        chunk(std::integral_constant<int, 0>{}, 0);
        chunk(std::integral_constant<int, 1>{}, 1);
        chunk(std::integral_constant<int, 2>{}, 2);
        chunk(std::integral_constant<int, 3>{}, 3);
        chunk(std::integral_constant<int, 4>{}, 4);
        chunk(std::integral_constant<int, 5>{}, 5);
#ifdef GPDE_V6_TIMING
        tm_peel += clock64() - tm0_;
#endif
        for (int c = 6; c < (IMAGE ? NKC - 1 : NKC); ++c) chunk(std::integral_constant<int, 6>{}, c);
        if constexpr (IMAGE) {
            chunk(std::integral_constant<int, 7>{}, NKC - 1);
            // The un-scale below is the first non-MFMA reader of the accumulators, and hipcc pads nothing behind an asm MFMA:
            // 16 wait states behind the last chunk's barrier (an 8-pass MFMA needs 12 before a VALU read of its D), then every
            // accumulator opaque, so that no v_accvgpr_read is hoisted across them into the K loop
            asm volatile("s_nop 15" ::: "memory");
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int nb = 0; nb < 8; ++nb) asm volatile("" : "+a"(acc[e][nb]));
        }

        TM_MARK(tm_loop);
        if constexpr (WRITE_H) {
            // ---- un-scale + bias + ReLU, store the tile's hidden activations (64-byte runs along the columns) ----
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const f32x4 ie = *(const f32x4*)&Es[16 * b + 4 * g];      // per-edge un-scale of this block's 4 accumulator rows
                auto store_rows = [&](auto full_tag) {
                    constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int e = e0 + 16 * b + 4 * g + r;
                        float* hp = a.hout + (size_t)(e - a.e_chunk0) * a.K2P + slice * GP_TN + l15;
#pragma unroll
                        for (int nb = 0; nb < 8; ++nb) {
                            const float y = fmaxf(fmaf(acc[b][nb][r], ie[r] * colc[GP_TN + nb * 16 + l15], colc[nb * 16 + l15]), 0.f);
                            acc[b][nb][r] = 0.f;
                            if (FULL || e < eb) { hp[nb * 16] = y; hmax_run = fmaxf(hmax_run, y); }
                        }
                    }
                };
                if (e0 + TE <= eb) store_rows(std::true_type{});
                else store_rows(std::false_type{});
            }
        } else
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            // H2 of the half's 32 edges as the aggregation's B operand: k slot (g, t) <-> edge 16 (t / 4) + 4g + t % 4 of the
            // half, which is the C layout of edge blocks 2b (t < 4) and 2b + 1 - the converted pairs are the operand as they are
            u4 g2hi[8], g2lo[8];
            float ie[8];            // per-edge un-scale of this half's 8 accumulator rows: two 16-byte LDS reads
#pragma unroll
            for (int q4 = 0; q4 < 2; ++q4) {
                const f32x4 t4 = *(const f32x4*)&Es[32 * b + 16 * q4 + 4 * g];
#pragma unroll
                for (int j = 0; j < 4; ++j) ie[4 * q4 + j] = t4[j];
            }
#pragma unroll
            for (int nb = 0; nb < 8; ++nb) {
                float y[8];
                const float b2v = colc[nb * 16 + l15], ucv = colc[GP_TN + nb * 16 + l15];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    y[r] = fmaf(acc[2 * b + (r >> 2)][nb][r & 3], ie[r] * ucv, b2v);
                    if constexpr (!IMAGE) acc[2 * b + (r >> 2)][nb][r & 3] = 0.f;
                }
#pragma unroll
                for (int p_ = 0; p_ < 4; ++p_) {
                    unsigned ph, pl;
                    conv_pair(y[2 * p_], y[2 * p_ + 1], ph, pl);
                    g2hi[nb][p_] = ph;
                    g2lo[nb][p_] = pl;
                }
                if (nb & 1) __builtin_amdgcn_sched_barrier(0);      // two column blocks at a time: 16 live values, not 64
            }
            const int s0 = e0 + 32 * b;
            const int s_end = min(s0 + 32, e_end);
            int e_seg = s0;
            const int n_last_b = __builtin_amdgcn_readfirstlane(nl_v[b]);
            int node = __builtin_amdgcn_readfirstlane(nf_v[b]);
            while (e_seg < s_end) {
                const int seg_end = (node == n_last_b) ? s_end : min(a.rowptr[node + 1], s_end);
                if (node != cur) {
                    if (cur >= 0) flush(cur);
                    cur = node;
                }
                const int lo = e_seg - s0 - 4 * g, hi = seg_end - s0 - 4 * g;
                const bool full = (e_seg == s0) && (seg_end == s0 + 32);       // the whole half is one segment (scalar)
                const unsigned* xu = Xs + 32 * b * GP_W;
                // four operand groups = channel blocks cb: 8 x_j words each (k slot tq <-> edge 16 (tq / 4) + tq % 4 + 4g of
                // the half, channel 16 cb + l15), read one group ahead of the 24 MFMAs that use them; ONE K = 32 MFMA covers
                // the half.  (The four lane groups read rows 4 apart = the same banks: a 2-way conflict on these 32 reads
                // per segment, against 96 MFMAs.)  The loads are unconditional and materialised by an asm before the masks:
                // hipcc otherwise sinks each load into its mask's branch and waits per word.
                unsigned wq[2][8];
                auto ldx = [&](int cb, unsigned (&w)[8]) {
#pragma unroll
                    for (int tq = 0; tq < 8; ++tq) {
                        const int er = 16 * (tq >> 2) + (tq & 3);
                        w[tq] = xu[(er + 4 * g) * GP_W + cb * 16 + l15];
                    }
                };
                ldx(0, wq[0]);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    unsigned (&w)[8] = wq[cb & 1];
                    if (cb + 1 < 4) ldx(cb + 1, wq[(cb + 1) & 1]);
                    asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]));
                    if (!full) {
#pragma unroll
                        for (int tq = 0; tq < 8; ++tq) {
                            const int er = 16 * (tq >> 2) + (tq & 3);
                            const unsigned keep = (er >= lo && er < hi) ? 0xffffffffu : 0u;
                            w[tq] &= keep;
                        }
                    }
                    u4 ah, al;
#pragma unroll
                    for (int jp = 0; jp < 4; ++jp) {
                        ah[jp] = __builtin_amdgcn_perm(w[2 * jp + 1], w[2 * jp], 0x05040100u);
                        al[jp] = __builtin_amdgcn_perm(w[2 * jp + 1], w[2 * jp], 0x07060302u);
                    }
                    const h8 xhi = __builtin_bit_cast(h8, ah), xlo = __builtin_bit_cast(h8, al);
#pragma unroll
                    for (int nb = 0; nb < 8; ++nb) {
                        const h8 gh = __builtin_bit_cast(h8, g2hi[nb]), gl = __builtin_bit_cast(h8, g2lo[nb]);
                        Z[cb][nb] = mfma32k(xhi, gh, Z[cb][nb]);
                        Z[cb][nb] = mfma32k(xhi, gl, Z[cb][nb]);
                        Z[cb][nb] = mfma32k(xlo, gh, Z[cb][nb]);
                        asm volatile("" : "+a"(Z[cb][nb]));      // Z stays in AGPRs (else: 128 copies per segment)
                    }
                }
                e_seg = seg_end;
                if (e_seg < s_end) node = a.dst[e_seg];
            }
        }
        if constexpr (MODE == 0)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int nb = 0; nb < 8; ++nb) asm volatile("" : "+a"(Z[cb][nb]));
        TM_MARK(tm_post);
        // ---- advance ---------------------------------------------------------------------------------------
        if constexpr (IMAGE) {
            float* es_t = Es;
            Es = Es_n;
            Es_n = es_t;
        }
        if (last_in_blk) {
            have = have_n;
            blk_a = na_;
            blk_b = nb_;
            e0 = have ? blk_a : e_hi;
        } else if (have) {
            e0 += TE;
        }
    }
    if constexpr (WRITE_H) {
        if (a.hmax_out) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) hmax_run = fmaxf(hmax_run, __shfl_xor(hmax_run, o));
            if (lane == 0 && hmax_run > 0.f) atomicMax(a.hmax_out, __float_as_uint(hmax_run));
        }
    } else if constexpr (MODE == 0) {
        if (cur >= 0) flush(cur);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef GPDE_V6_TIMING
    if (lane == 0) {
        atomicAdd(&gpde_v6_tm[0], (unsigned long long)tm_pro);
        atomicAdd(&gpde_v6_tm[1], (unsigned long long)tm_loop);
        atomicAdd(&gpde_v6_tm[2], (unsigned long long)tm_post);
        atomicAdd(&gpde_v6_tm[3], (unsigned long long)n_rounds);
        atomicAdd(&gpde_v6_tm[4], (unsigned long long)tm_peel);
    }
#endif
}

size_t v6_lds_bytes(int K1P) {
    return (size_t)NS * TILE_B + (size_t)K1P * 32 + (size_t)NW * TE * GP_W * 4 + (size_t)NW * TE * 4 + 64 +
           2 * GP_TN * 4;       // (+ 1 KiB: the per-column bias and un-scale factor of the slice, `colc`)
}
// the image variant: + a 2 KiB staging area and a second `Es` per wave
size_t v6_image_lds_bytes(int K1P) { return v6_lds_bytes(K1P) + (size_t)NW * 2048 + (size_t)NW * TE * 4; }

}  // namespace

#ifdef GPDE_V6_TIMING
extern "C" GPDE_API int gpde_debug_v6_timing(unsigned long long* out8, int reset) {
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(gpde_v6_tm), 64) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(gpde_v6_tm), z, 64) != hipSuccess) return -1;
    }
    return 0;
}
#endif

// 3-Linear kernels with at least 8 k1 chunks (the side loads of a tile are spread over its first seven), attributes +
// bias slot within one K = 8 group, split-x input (a.xs) present
bool gpde_fused_f16v6_supported(const GpdeFusedArgs& a) {
    return a.K1P / GP_BK >= 8 && a.k0 + 1 <= 8 && v6_lds_bytes(a.K1P) <= 160 * 1024 &&
           (a.hout != nullptr || a.xs != nullptr);
}

// The image variant's shapes: the kernel's, with room for its staging areas (K1P up to 1152).  Wider ones keep the
// per-tile prologue - the same kernel, not the 8-wave one
bool gpde_fused_f16v6_image_supported(const GpdeFusedArgs& a) {
    GpdeFusedArgs p = a;
    if (!p.xs) p.xs = (const unsigned*)(uintptr_t)8;      // "will be present"
    p.hout = nullptr;
    return gpde_fused_f16v6_supported(p) && v6_image_lds_bytes(a.K1P) <= 160 * 1024;
}

int gpde_launch_fused_f16v6(const GpdeFusedArgs& a, hipStream_t stream) {
    const int ns = a.K2P / GP_TN;
    const dim3 grid(a.n_groups * ns), block(256);
    const size_t lds = v6_lds_bytes(a.K1P);
    static GpdeLdsOnce once;
    if (int rc = once.ensure(gpde_fused_f16v6_kernel<0, ASRC_TENSOR>, gpde_fused_f16v6_kernel<1, ASRC_TENSOR>,
                             gpde_fused_f16v6_kernel<0, ASRC_NODES>, gpde_fused_f16v6_kernel<1, ASRC_NODES>,
                             gpde_fused_f16v6_kernel<0, ASRC_IMAGE>)) return rc;
    if (a.hout) {
        GpdeFusedArgs b = a;
        b.blk = nullptr; b.qn = nullptr; b.qctr = nullptr;             // rows are independent: static ranges
        if (a.kt) hipLaunchKernelGGL((gpde_fused_f16v6_kernel<1, ASRC_NODES>), grid, block, lds, stream, b);     // row f3 in training
        else hipLaunchKernelGGL((gpde_fused_f16v6_kernel<1, ASRC_TENSOR>), grid, block, lds, stream, b);
    } else if (a.img_hi) {
        if (!a.img_lo || !a.img_isc || !a.img_rec || !gpde_fused_f16v6_image_supported(a)) {
            gpde_set_error("gpde_fused_f16v6_kernel: attribute image incomplete or K1P = %d beyond the image variant", a.K1P);
            return GPDE_EINVAL;
        }
        hipLaunchKernelGGL((gpde_fused_f16v6_kernel<0, ASRC_IMAGE>), grid, block, v6_image_lds_bytes(a.K1P), stream, a);
    } else if (a.kt) hipLaunchKernelGGL((gpde_fused_f16v6_kernel<0, ASRC_NODES>), grid, block, lds, stream, a);
    else hipLaunchKernelGGL((gpde_fused_f16v6_kernel<0, ASRC_TENSOR>), grid, block, lds, stream, a);
    GP_LAUNCH_CHECK("gpde_fused_f16v6_kernel");
    return GPDE_OK;
}

// The store variant of the fused kernel (H rows instead of the aggregation): the one-wave-per-SIMD kernel where its
// shape is covered (>= 8 k1 chunks), else the 8-wave kernel.
bool gpde_fused_store_supported(GpdeFusedArgs probe) {
    if (!probe.hout) probe.hout = (float*)(uintptr_t)8;      // "will be present"
    return gpde_fused_f16v6_supported(probe) || gpde_fused_f16v3_supported(probe);
}

int gpde_launch_fused_store(const GpdeFusedArgs& f, hipStream_t stream) {
    if (!f.hout) { gpde_set_error("gpde_launch_fused_store: hout is null"); return GPDE_EINVAL; }
    if (gpde_fused_f16v6_supported(f)) return gpde_launch_fused_f16v6(f, stream);
    if (gpde_fused_f16v3_supported(f)) return gpde_launch_fused_f16v3(f, stream);
    gpde_set_error("fused store kernel: unsupported kernel MLP (K1P = %d, k0 = %d)", f.K1P, f.k0);
    return GPDE_EUNSUPPORTED;
}
