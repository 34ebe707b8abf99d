// Model of the v6 K loop: FOUR waves per workgroup (one per SIMD, up to 512 registers each), wave tile
// 64 edges x 128 hidden columns, in two MFMA shapes (template parameter SHAPE).
// SHAPE 0, v_mfma_f32_32x32x16_f16 (the kernel up to the shape change).  Per 32-wide k chunk and wave: 48 f16 MFMAs
// (2 edge blocks x 4 column blocks x 2 k16 steps x 3 split products) + 4 H1 MFMAs, 16 ds_read_b128 of W2 fragments,
// 2 of (W1|b1), 16 conversion pairs (5 VALU each), 4 LDS-DMA pieces of the next W2 chunk image, one s_barrier.
// SHAPE 1, v_mfma_f32_16x16x32_f16 (the kernel now): 96 + 8 MFMAs of half the size, everything else the same (body16).
// SHAPE 2: the same MFMAs in the kernel's LEVELLED schedule (body16<.., LV = 1>: half-chunk-major, one conversion instruction per gap).
// SHAPE 3: the levelled schedule with FOUR RESIDENT fragment sets (body16<.., LV = 2>): every W2 fragment is read once per chunk.
// SHAPE 4: SHAPE 3 as a PEELED chunk of the image variant (body16<.., LV = 3>): + the side loads of chunks 3-5 (four ds_bpermute of the
//          x_j row addresses, four gather LDS-DMA of x_j rows, closing wait vmcnt(4)), accumulators tied (D = C) as everywhere in this model.
// SHAPE 5: SHAPE 4 + the accumulator copies hipcc puts into the kernel's peeled chunks (body16<.., LV = 4>): four accumulators per chunk
//          parked in VGPRs behind their first product (s_nop 7, 4 v_accvgpr_read_b32) and put back in front of their second
//          (4 v_accvgpr_write_b32, s_nop 1) - 32 copies and 8 pads per chunk against the kernel's 33 and 15.
// Flags ablate the parts; the result is cycles per chunk (ideal 52 x 32 = 104 x 16 = 1664), the shader clock and chip
// TFLOP/s.  The run ends with the shape A/B (bare stream and full model of both shapes, alternating, in long launches) and
// the schedule A/B (full model, SHAPE 1 against SHAPE 2), the fragment A/B (full model, SHAPE 2 against SHAPE 3) and the copy A/B
// (peeled chunk with side loads, SHAPE 4 against SHAPE 5: what the accumulator copies of a peeled chunk cost).
//   hipcc --offload-arch=gfx950 -O3 -o kloop_model_v6 kloop_model_v6.hip && ./kloop_model_v6        (./kloop_model_v6 copy: the copy A/B alone)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void dma16(const void* gsrc, void* lds) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}
__device__ __forceinline__ f32x16 mfma16(h8 a, h8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float relu1(float v) { return __int_as_float(max(__float_as_int(v), 0)); }

constexpr int TILE_B = 16384;
// FLAGS: 1 conversions, 2 barrier, 4 W2 DMA ring + counted wait, 8 H1 MFMAs, 16 W2 fragment reads,
//        32 keep 128 extra accumulator registers (Z) live across the loop, 64 H1 MFMAs by asm into VGPRs
// NS: ring slots (3: DMA one chunk ahead, vmcnt(0) per chunk; 4: two chunks ahead, vmcnt(4))
template <int FLAGS, int NS>
__device__ __forceinline__ void body32(char* smem, long* out, const char* gsrc, float seed, int iters) {
    char* ring = smem;
    char* w1s = smem + NS * TILE_B;           // 32 KiB
    for (int i = threadIdx.x; i < (NS * TILE_B + 32768) / 4; i += 256) ((float*)smem)[i] = (float)((i * 2654435761u) >> 20) * 1e-3f;
    __syncthreads();
    const int lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sw = (l31 >> 1) & 7;
    const int rowb = l31 * 128;
    const int boff[2] = {rowb + (((0 + h) ^ sw) << 4), rowb + (((2 + h) ^ sw) << 4)};

    u4 ahi[2][2], alo[2][2];
    h8 bhi[4], blo[4], B1[2], B2[2];
    f32x16 d[2], acc[2][4], Z[2][4];
    for (int b = 0; b < 2; ++b)
        for (int e = 0; e < 2; ++e)
            for (int j = 0; j < 4; ++j) {
                // pseudo-random f16 pairs per lane / register (sign + 12 random low bits on exponent 0x30..0x3f: magnitudes 0.1 .. 2;
                // lo parts 2^-11 of that): the power draw of an MFMA depends on the operand bits (round 4: was a near-constant)
                unsigned r_ = (unsigned)(lane * 2654435761u) ^ (unsigned)((b * 8 + e * 4 + j + 1) * 40503u) ^ (unsigned)(blockIdx.x * 97u);
                r_ = r_ * 1664525u + 1013904223u;
                const unsigned h0 = 0x3000u + ((r_ >> 4) & 0x0fffu) + ((r_ >> 1) & 0x8000u), h1 = 0x3000u + ((r_ >> 18) & 0x0fffu) + ((r_ << 3) & 0x8000u);
                ahi[b][e][j] = h0 | (h1 << 16);
                alo[b][e][j] = (0x0400u + ((r_ >> 9) & 0x0fffu)) | ((0x0400u + ((r_ >> 13) & 0x0fffu) + ((r_ << 7) & 0x8000u)) << 16);
            }
    for (int e = 0; e < 2; ++e)
        for (int j = 0; j < 8; ++j) { B1[e][j] = (_Float16)(seed + j * 0.1f + e); B2[e][j] = (_Float16)(seed - j * 0.1f); }
    for (int e = 0; e < 2; ++e)
        for (int nb = 0; nb < 4; ++nb)
            for (int r = 0; r < 16; ++r) { acc[e][nb][r] = 0.f; Z[e][nb][r] = seed * r; }
    for (int e = 0; e < 2; ++e)
        for (int r = 0; r < 16; ++r) d[e][r] = seed * (r + 1) * 0.01f;
    for (int nb = 0; nb < 4; ++nb) { bhi[nb] = *(const h8*)(ring + nb * 4096 + boff[0]); blo[nb] = *(const h8*)(ring + nb * 4096 + (boff[0] ^ 64)); }

    const unsigned long long gbase = (unsigned long long)gsrc + (size_t)(blockIdx.x % 8) * 32 * TILE_B + wave * 4096;
    const unsigned lane16 = lane * 16;
    // the 4 pieces of a wave are 1 KiB apart in the global image AND in the LDS slot: one address, the
    // instruction's immediate offset advances both sides
    auto issue_w2 = [&](int chunk, int slot, int piece) {
        unsigned long long gb = gbase + (size_t)chunk * TILE_B;
        asm volatile("" : "+s"(gb));
        const char* g = (const char*)(gb + lane16);
        char* l = ring + slot * TILE_B + wave * 4096;
        if (piece == 0) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
        if (piece == 1) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 1024, 0);
        if (piece == 2) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 2048, 0);
        if (piece == 3) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 3072, 0);
    };
    // one asm statement per conversion pair (relu, hi = rtz16, lo = rn16(y - hi)): a single compiler
    // boundary pad instead of one per instruction.  The inputs are MFMA results: the H1 MFMAs are placed
    // >= 3 MFMAs before the first conversion that reads them (hipcc pads nothing for asm operands).
    auto conv_a = [&](const f32x16& v, int m, int jp, unsigned& ph, unsigned& t0_, unsigned& t1_) {
        asm("v_max_i32 %1, 0, %3\n\t"
            "v_max_i32 %2, 0, %4\n\t"
            "v_cvt_pkrtz_f16_f32 %0, %1, %2"
            : "=&v"(ph), "=&v"(t0_), "=&v"(t1_) : "v"(v[8 * m + 2 * jp]), "v"(v[8 * m + 2 * jp + 1]));
    };
    auto conv_b = [&](int jp, unsigned ph, unsigned t0_, unsigned t1_, u4& hi, u4& lo) {
        unsigned pl;
        asm("v_fma_mixlo_f16 %0, %1, 1.0, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixhi_f16 %0, %2, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
            : "=&v"(pl) : "v"(t0_), "v"(t1_), "v"(ph));
        hi[jp] = ph;
        lo[jp] = pl;
    };
    // H1 MFMA with a VGPR destination (the builtin lands in AGPRs in a 512-register kernel and every value
    // then costs a v_accvgpr_read before the conversion)
    auto h1gen = [&](f32x16& dd, h8 a1, h8 a2, h8 b1, h8 b2) {
        if (FLAGS & 64) {
            asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(dd) : "v"(a1), "v"(b1));
            asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(dd) : "v"(a2), "v"(b2));
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) dd[r] = 0.f;
            dd = mfma16(a1, b1, dd);
            dd = mfma16(a2, b2, dd);
        }
    };

    if (FLAGS & 4) {
        for (int p = 0; p < 4; ++p) issue_w2(1, 1, p);
        if (NS == 4) for (int p = 0; p < 4; ++p) issue_w2(2, 2, p);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (FLAGS & 32) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) asm volatile("" : "+a"(Z[e][nb]));
    }
    int slot = 0;
    unsigned cph = 0, ct0 = 0, ct1 = 0;
    h8 A1 = *(const h8*)(w1s + l31 * 32), A2 = *(const h8*)(w1s + l31 * 32 + 16);
    long t0 = clock64();
    for (int it = 0; it < iters; ++it) {
        int slot1 = slot + 1 == NS ? 0 : slot + 1;            // next chunk's slot
        int slot2 = slot1 + 1 == NS ? 0 : slot1 + 1;
        int slot3 = slot2 + 1 == NS ? 0 : slot2 + 1;
        const int dslot = NS == 3 ? slot2 : slot3;            // DMA target: chunk it+2 (3 slots) / it+3 (4 slots)
        const int dchunk = (it + (NS == 3 ? 2 : 3)) & 31;
        const char* rb0 = ring + slot * TILE_B;
        const char* rb1 = ring + slot1 * TILE_B;
        const char* w1n = w1s + (size_t)((((it + 1) & 31) * 32) + l31) * 32;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int cb = m;              // operand buffer of this step; the next step's is cb ^ 1
            // where the NEXT step's B fragments live
            const char* rn = (m == 0) ? rb0 : rb1;
            const int bo = boff[m ^ 1];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const int t = j >> 1, e = j & 1;
                    const int i = nb * 6 + j;
                    if (!((FLAGS & 128) && t == 2))       // flag 128: two of the three split products (what less matrix work per edge would buy)
                        acc[e][nb] = mfma16(__builtin_bit_cast(h8, t == 2 ? alo[cb][e] : ahi[cb][e]), t == 0 ? blo[nb] : bhi[nb], acc[e][nb]);
                    asm volatile("" : "+a"(acc[e][nb]));
                    // conversion pair p of the next step's operands: first part (relu, relu, hi) after MFMA 3p,
                    // second part (lo) after MFMA 3p + 1.  In step 1 the raw H1 of the next chunk was issued at
                    // the end of step 0: everything one MFMA later (pair 7 after MFMAs 22 / 23).
                    {
                        const int q = m == 0 ? i : i - 1;
                        if ((FLAGS & 1) && q >= 0 && q % 3 == 0 && q / 3 < 8) conv_a(d[(q / 3) >> 2], m ^ 1, (q / 3) & 3, cph, ct0, ct1);
                        if ((FLAGS & 1) && q >= 0 && q % 3 == 1 && q / 3 < 8) {
                            conv_b((q / 3) & 3, cph, ct0, ct1, ahi[cb ^ 1][(q / 3) >> 2], alo[cb ^ 1][(q / 3) >> 2]);
                            asm volatile("" ::"v"(ahi[cb ^ 1][(q / 3) >> 2]), "v"(alo[cb ^ 1][(q / 3) >> 2]));
                        }
                    }
                    if (FLAGS & 16) {
                        if (j == 1) blo[nb] = *(const h8*)(rn + nb * 4096 + (bo ^ 64));
                        if (j == 5) bhi[nb] = *(const h8*)(rn + nb * 4096 + bo);
                    }
                    if ((FLAGS & 4) && m == 0 && (i == 2 || i == 8 || i == 14 || i == 20)) issue_w2(dchunk, dslot, (i - 2) / 6);
                    if ((FLAGS & 8) && m == 0 && i == 4) A1 = *(const h8*)w1n;
                    if ((FLAGS & 8) && m == 0 && i == 10) A2 = *(const h8*)(w1n + 16);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (m == 0 && (FLAGS & 8)) {
                // H1 of the next chunk (single-buffered raw H1: its last reader ran just above)
                h1gen(d[0], A1, A2, B1[0], B2[0]);
                h1gen(d[1], A1, A2, B1[1], B2[1]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (FLAGS & 4) {
            if (NS == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");       // this chunk's 4 pieces stay in flight
        }
        if (FLAGS & 2) __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        slot = slot1;
    }
    long t1 = clock64();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (FLAGS & 32) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) asm volatile("" : "+a"(Z[e][nb]));
    }
    float s = 0;
    for (int e = 0; e < 2; ++e)
        for (int nb = 0; nb < 4; ++nb)
            for (int r = 0; r < 16; ++r) s += acc[e][nb][r] + ((FLAGS & 32) ? Z[e][nb][r] : 0.f);
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = t1 - t0;
    if (s == 1234.5f) out[1] = 1;
}

// The same K loop on v_mfma_f32_16x16x32_f16 (SHAPE 1; since the kernel moved to this shape, the one it runs): same 64 x 128 wave
// tile as 4 edge blocks x 8 column blocks of f32x4, ONE k32 step per chunk.  A chunk is four batches of two column blocks,
// per batch the edge blocks 0..3 with 2 column blocks x 3 split products = 6 MFMAs each: 96 product MFMAs + 8 H1 MFMAs
// (one per edge block and 16-row half: the three split terms of H1 sit in the lane groups of one K = 32 MFMA).  The 32
// fragment registers are two sets of one batch (hi + lo of two column blocks); the next batch's set is read during the
// current batch.  The operands are SINGLE-buffered (32 registers): the next chunk's edge block e is converted into the
// registers of edge block e from the gap behind its last MFMA on, eight gaps each, wrapping into the next chunk's first
// 14 gaps.  Same 16 ds_read_b128 of W2 fragments (unit g = lane / 16 of the unchanged chunk image), 2 of (W1|b1), 16
// conversion pairs, 4 DMA pieces, one s_barrier; at most 4 non-MFMA instructions per gap.  Ideal 104 x 16 = 1664 cycles
// per chunk, as for the 32x32 loop.  (A first form with two batches of four column blocks, the next batch's fragments
// re-read in place during the batch's last edge block, measured 2241 cycles per chunk against this one's 2224.)
//
// LV 1, the LEVELLED schedule (half-chunk-major): edge blocks {0, 1} run over all eight column blocks (MFMAs 0..47), then edge
// blocks {2, 3} (48..95); inside a half the same four batches of two column blocks, so every accumulator still receives hi x lo,
// hi x hi, lo x hi in that order.  A half leaves the other half's operand registers free for 48 gaps: the next operands of edge
// blocks {2, 3} are converted in gaps 0..46, those of {0, 1} in gaps 48..94, ONE conversion instruction per gap (five
// single-instruction asm statements per pair).  The W2 fragments are read twice per chunk (32 ds_read_b128, one per three gaps,
// into the other set as before); gaps 5, 11, .. (two per batch) carry no conversion and take the DMA pieces (5, 11, 17, 23);
// the (W1|b1) reads ride in gaps 25, 31.  Raw H1 comes in two halves of four MFMAs: edge blocks {0, 1} of the next chunk behind
// MFMA 45, {2, 3} behind MFMA 93, each two MFMAs ahead of its first conversion.  No gap carries more than two instructions.
//
// LV 2, the levelled schedule with RESIDENT fragments: four sets of 16 registers, batch bt of either half reads set bt, so no
// fragment is read twice in a chunk (16 ds_read_b128, none in the first half but set 3).  The next chunk's sets 0, 1, 2 are read
// from its ring slot during the second half's batches 1, 2, 3 - each behind the set's last reader of this chunk and a batch or
// more ahead of its first reader of the next - and set 3 during the next chunk's own first batch.  Same gaps (q = 0, 3, 6, 9).
//
// LV 3, LV 2 as a peeled chunk of the image variant (its chunks 3, 4, 5): the x_j row addresses by ds_bpermute in gaps 1, 7, 13, 19, the
// four gather DMA of x_j rows in gaps 53, 65, 77, 89 (behind the ring pieces), and the closing wait leaves those four in flight.
// LV 4, LV 3 with accumulator copies as hipcc places them around the side loads: the accumulator of MFMA 48, 60, 72, 84 (the first product
// of a batch) is read into VGPRs behind it (s_nop 7 first: MFMA result -> VALU read) and written back in the next gap, in front of the
// second product into it (s_nop 1 behind: VALU write -> MFMA C).  The values come back unchanged.
template <int FLAGS, int NS, int LV = 0>
__device__ __forceinline__ void body16(char* smem, long* out, const char* gsrc, float seed, int iters) {
    char* ring = smem;
    char* w1s = smem + NS * TILE_B;           // 32 KiB
    for (int i = threadIdx.x; i < (NS * TILE_B + 32768) / 4; i += 256) ((float*)smem)[i] = (float)((i * 2654435761u) >> 20) * 1e-3f;
    __syncthreads();
    const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // chunk image row = hidden column (128 B: units 0-3 hi k 0-7 | 8-15 | 16-23 | 24-31, units 4-7 lo), unit position
    // swizzled by (column >> 1) & 7; a column block is 16 rows = 2 KiB
    const int bo = l15 * 128 + ((g ^ ((l15 >> 1) & 7)) << 4);
    // (W1|b1) row of D row l15 for half 0 (half 1: 8 rows on; the k order of the pack's units); lane group 2 reads the lo
    // 16 bytes, the others the hi
    const int w1o = (16 * (l15 >> 3) + 4 * ((l15 >> 2) & 1) + (l15 & 3)) * 32 + (g == 2 ? 16 : 0);

    u4 ahi[4], alo[4];
    constexpr int NFS = LV >= 2 ? 4 : 2;      // fragment sets
    h8 bhi[NFS][2], blo[NFS][2], B1[4];
    f32x4 d[4][2], acc[4][8], Z[4][8];
    for (int e = 0; e < 4; ++e)
        for (int j = 0; j < 4; ++j) {
            // the same pseudo-random f16 pairs as the 32x32 body
            unsigned r_ = (unsigned)(lane * 2654435761u) ^ (unsigned)((e * 4 + j + 1) * 40503u) ^ (unsigned)(blockIdx.x * 97u);
            r_ = r_ * 1664525u + 1013904223u;
            const unsigned h0 = 0x3000u + ((r_ >> 4) & 0x0fffu) + ((r_ >> 1) & 0x8000u), h1 = 0x3000u + ((r_ >> 18) & 0x0fffu) + ((r_ << 3) & 0x8000u);
            ahi[e][j] = h0 | (h1 << 16);
            alo[e][j] = (0x0400u + ((r_ >> 9) & 0x0fffu)) | ((0x0400u + ((r_ >> 13) & 0x0fffu) + ((r_ << 7) & 0x8000u)) << 16);
        }
    // attributes: hi | lo | hi | zero by lane group
    for (int e = 0; e < 4; ++e)
        for (int j = 0; j < 8; ++j) B1[e][j] = g == 3 ? (_Float16)0.f : (_Float16)(g == 1 ? (seed - j * 0.1f) * 4.8828125e-4f : seed + j * 0.1f + e);
    for (int e = 0; e < 4; ++e)
        for (int nb = 0; nb < 8; ++nb)
            for (int r = 0; r < 4; ++r) { acc[e][nb][r] = 0.f; Z[e][nb][r] = seed * (r + 4 * (nb & 3)); }
    for (int e = 0; e < 4; ++e)
        for (int hf = 0; hf < 2; ++hf)
            for (int r = 0; r < 4; ++r) d[e][hf][r] = seed * (4 * hf + r + 1) * 0.01f;
    for (int nb = 0; nb < 2; ++nb) { bhi[0][nb] = *(const h8*)(ring + nb * 2048 + bo); blo[0][nb] = *(const h8*)(ring + nb * 2048 + (bo ^ 64)); bhi[1][nb] = bhi[0][nb]; blo[1][nb] = blo[0][nb]; }
    if constexpr (LV >= 2)
        for (int s = 2; s < 4; ++s)
            for (int nb = 0; nb < 2; ++nb) { bhi[s][nb] = *(const h8*)(ring + (2 * s + nb) * 2048 + bo); blo[s][nb] = *(const h8*)(ring + (2 * s + nb) * 2048 + (bo ^ 64)); }

    const unsigned long long gbase = (unsigned long long)gsrc + (size_t)(blockIdx.x % 8) * 32 * TILE_B + wave * 4096;
    const unsigned lane16 = lane * 16;
    auto issue_w2 = [&](int chunk, int slot, int piece) {
        unsigned long long gb = gbase + (size_t)chunk * TILE_B;
        asm volatile("" : "+s"(gb));
        const char* gp = (const char*)(gb + lane16);
        char* l = ring + slot * TILE_B + wave * 4096;
        if (piece == 0) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
        if (piece == 1) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp, (__attribute__((address_space(3))) void*)l, 16, 1024, 0);
        if (piece == 2) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp, (__attribute__((address_space(3))) void*)l, 16, 2048, 0);
        if (piece == 3) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp, (__attribute__((address_space(3))) void*)l, 16, 3072, 0);
    };
    // the conversion pair of the 32x32 body.  After the two halves a lane holds k = 8g .. 8g+7 of its edge (half hf gives
    // k = 8g + 4 hf + r): pair jp = values 2 jp, 2 jp + 1 = d[e][jp >> 1][2 (jp & 1) ..]
    auto conv_a = [&](float v0, float v1, unsigned& ph, unsigned& t0_, unsigned& t1_) {
        asm("v_max_i32 %1, 0, %3\n\t"
            "v_max_i32 %2, 0, %4\n\t"
            "v_cvt_pkrtz_f16_f32 %0, %1, %2"
            : "=&v"(ph), "=&v"(t0_), "=&v"(t1_) : "v"(v0), "v"(v1));
    };
    auto conv_b = [&](int jp, unsigned ph, unsigned t0_, unsigned t1_, u4& hi, u4& lo) {
        unsigned pl;
        asm("v_fma_mixlo_f16 %0, %1, 1.0, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixhi_f16 %0, %2, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
            : "=&v"(pl) : "v"(t0_), "v"(t1_), "v"(ph));
        hi[jp] = ph;
        lo[jp] = pl;
    };
    // ONE H1 MFMA per edge block and half: K = 32 carries W1hi x attr_hi + W1hi x attr_lo + W1lo x attr_hi
    auto h1gen = [&](f32x4& dd, h8 a, h8 b) {
        if (FLAGS & 64) {
            asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(dd) : "v"(a), "v"(b));
        } else {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            dd = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, z, 0, 0, 0);
        }
    };
    // LV 1: the conversion pair as five statements of one instruction (step 0..4), one per MFMA gap
    auto conv_step = [&](int step, float v0, float v1, unsigned& ph, unsigned& t0_, unsigned& t1_, unsigned& pl) {
        if (step == 0) asm("v_max_i32 %0, 0, %1" : "=v"(t0_) : "v"(v0));
        if (step == 1) asm("v_max_i32 %0, 0, %1" : "=v"(t1_) : "v"(v1));
        if (step == 2) asm("v_cvt_pkrtz_f16_f32 %0, %1, %2" : "=v"(ph) : "v"(t0_), "v"(t1_));
        if (step == 3) asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(pl) : "v"(t0_), "v"(ph));
        if (step == 4) asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(pl) : "v"(t1_), "v"(ph));
    };

    if (FLAGS & 4) {
        for (int p = 0; p < 4; ++p) issue_w2(1, 1, p);
        if (NS == 4) for (int p = 0; p < 4; ++p) issue_w2(2, 2, p);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (FLAGS & 32) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nb = 0; nb < 8; ++nb) asm volatile("" : "+a"(Z[e][nb]));
    }
    int slot = 0;
    unsigned cph = 0, ct0 = 0, ct1 = 0, cpl = 0;
    h8 A1 = *(const h8*)(w1s + w1o), A2 = *(const h8*)(w1s + w1o + 256);
    // LV >= 3: the wave's x_j piece (4 DMA of 4 rows x 256 B) behind the (W1|b1) rows; source rows picked per lane and chunk
    [[maybe_unused]] char* xs = smem + NS * TILE_B + 32768 + wave * 4096;
    [[maybe_unused]] int xsidx[4] = {0, 0, 0, 0};
    [[maybe_unused]] int src_l = (int)(lane * 2654435761u >> 18);
    [[maybe_unused]] float pk[4];
    long t0 = clock64();
    for (int it = 0; it < iters; ++it) {
        int slot1 = slot + 1 == NS ? 0 : slot + 1;            // next chunk's slot
        int slot2 = slot1 + 1 == NS ? 0 : slot1 + 1;
        int slot3 = slot2 + 1 == NS ? 0 : slot2 + 1;
        const int dslot = NS == 3 ? slot2 : slot3;            // DMA target: chunk it+2 (3 slots) / it+3 (4 slots)
        const int dchunk = (it + (NS == 3 ? 2 : 3)) & 31;
        const char* rb0 = ring + slot * TILE_B;
        const char* rb1 = ring + slot1 * TILE_B;
        const char* w1n = w1s + (size_t)(((it + 1) & 31) * 32) * 32 + w1o;
        if constexpr (LV >= 3) src_l += 40503 * it;
        if constexpr (LV >= 1) {
            unsigned long long gb_c = gbase + (size_t)dchunk * TILE_B;
            asm volatile("" : "+s"(gb_c));
            const char* gp_c = (const char*)(gb_c + lane16);
#pragma unroll
            for (int g8 = 0; g8 < 8; ++g8) {            // batch of the chunk: half hf, column blocks 2 bt, 2 bt + 1
                const int hf = g8 >> 2, bt = g8 & 3, fs = LV >= 2 ? bt : (g8 & 1);
                // the NEXT batch's fragments: the next column blocks of this chunk (0, 1 again behind the first half), then 0, 1 of
                // the next chunk, into the other set.  LV 2: set rs, or none (rs < 0) - set 3 of this chunk in the first batch, sets
                // bt - 1 of the next chunk in the second half's batches bt = 1, 2, 3
                const int rs = LV < 2 ? (fs ^ 1) : (g8 == 0 ? 3 : (g8 >= 5 ? bt - 1 : -1));
                const char* rn = LV >= 2 ? (g8 == 0 ? rb0 + 6 * 2048 : rb1 + (2 * (bt - 1)) * 2048)
                                         : ((g8 < 7) ? rb0 + (2 * ((bt + 1) & 3)) * 2048 : rb1);
#pragma unroll
                for (int q = 0; q < 12; ++q) {
                    const int e = 2 * hf + q / 6, i = q % 6;
                    const int t = i >> 1, nb = i & 1;
                    const int cbk = 2 * bt + nb;
                    const int n = g8 * 12 + q;              // MFMA index in the chunk
                    if (!((FLAGS & 128) && t == 2))
                        acc[e][cbk] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, t == 2 ? alo[e] : ahi[e]), t == 0 ? blo[fs][nb] : bhi[fs][nb], acc[e][cbk], 0, 0, 0);
                    asm volatile("" : "+a"(acc[e][cbk]));
                    // conversions of the OTHER half's edge blocks (first half: this chunk's {2, 3}, second half: the next chunk's
                    // {0, 1}): batch bt converts pairs 2 bt, 2 bt + 1 of the eight, one instruction per gap, none in gaps 5 and 11
                    if ((FLAGS & 1) && q != 5 && q != 11) {
                        const int v = q < 5 ? q : q - 1, pr = 2 * bt + v / 5, step = v % 5;
                        const int ce = 2 * (1 - hf) + (pr >> 2), jp = pr & 3;
                        conv_step(step, d[ce][jp >> 1][2 * (jp & 1)], d[ce][jp >> 1][2 * (jp & 1) + 1], cph, ct0, ct1, cpl);
                        if (step == 4) {
                            ahi[ce][jp] = cph;
                            alo[ce][jp] = cpl;
                        }
                    } else if (FLAGS & 1) {
                        // keeps the converted registers live in the model; a gap behind their last write (read by an asm in
                        // the same gap as the write, hipcc pads an s_nop in front of the next MFMA)
                        const int ce = 2 * (1 - hf) + (bt >> 1);
                        asm volatile("" ::"v"(ahi[ce]), "v"(alo[ce]));
                    }
                    if ((FLAGS & 16) && rs >= 0) {          // the other set's last reader was the previous batch
                        if (q == 0) blo[rs][0] = *(const h8*)(rn + (bo ^ 64));
                        if (q == 3) blo[rs][1] = *(const h8*)(rn + 2048 + (bo ^ 64));
                        if (q == 6) bhi[rs][0] = *(const h8*)(rn + bo);
                        if (q == 9) bhi[rs][1] = *(const h8*)(rn + 2048 + bo);
                    }
                    if ((FLAGS & 4) && n < 24 && q % 6 == 5) {           // one address per chunk (gp_c), immediate offsets
                        char* l = ring + dslot * TILE_B + wave * 4096;
                        if (n == 5) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp_c, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
                        if (n == 11) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp_c, (__attribute__((address_space(3))) void*)l, 16, 1024, 0);
                        if (n == 17) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp_c, (__attribute__((address_space(3))) void*)l, 16, 2048, 0);
                        if (n == 23) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp_c, (__attribute__((address_space(3))) void*)l, 16, 3072, 0);
                    }
                    if ((FLAGS & 8) && n == 25) A1 = *(const h8*)w1n;
                    if ((FLAGS & 8) && n == 31) A2 = *(const h8*)(w1n + 256);
                    if constexpr (LV >= 3) {
                        // the side loads of a peeled chunk: row i = 0..3 of this chunk's x_j piece, 4 rows of 256 B per DMA
                        if (n == 1 || n == 7 || n == 13 || n == 19)
                            xsidx[(n - 1) / 6] = __builtin_amdgcn_ds_bpermute((4 * ((n - 1) / 6) + (lane >> 4)) * 4, src_l);
                        if (n == 53 || n == 65 || n == 77 || n == 89)
                            dma16(gsrc + (size_t)(xsidx[(n - 53) / 12] & 0x3fff) * 256 + (lane & 15) * 16, xs + ((n - 53) / 12) * 1024);
                    }
                    if constexpr (LV == 4) {
                        if (q == 0 && hf == 1)          // park the accumulator MFMA n has just written
                            asm volatile("s_nop 7\n\tv_accvgpr_read_b32 %0, %4\n\tv_accvgpr_read_b32 %1, %5\n\t"
                                         "v_accvgpr_read_b32 %2, %6\n\tv_accvgpr_read_b32 %3, %7"
                                         : "=&v"(pk[0]), "=&v"(pk[1]), "=&v"(pk[2]), "=&v"(pk[3])
                                         : "a"(acc[e][cbk][0]), "a"(acc[e][cbk][1]), "a"(acc[e][cbk][2]), "a"(acc[e][cbk][3]));
                        if (q == 1 && hf == 1) {        // and put it back in front of MFMA n + 1, its second product
                            f32x4& ac = acc[e][2 * bt];
                            asm volatile("v_accvgpr_write_b32 %0, %4\n\tv_accvgpr_write_b32 %1, %5\n\t"
                                         "v_accvgpr_write_b32 %2, %6\n\tv_accvgpr_write_b32 %3, %7\n\ts_nop 1"
                                         : "=a"(ac[0]), "=a"(ac[1]), "=a"(ac[2]), "=a"(ac[3])
                                         : "v"(pk[0]), "v"(pk[1]), "v"(pk[2]), "v"(pk[3]));
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if ((FLAGS & 8) && (n == 45 || n == 93)) {
                        // raw H1 of the next chunk, edge blocks {0, 1} / {2, 3}: the last reader of these registers (the
                        // conversions of the other half) ran a gap earlier, the first reader is two MFMAs on
                        const int e0 = n == 45 ? 0 : 2;
                        h1gen(d[e0][0], A1, B1[e0]); h1gen(d[e0][1], A2, B1[e0]);
                        h1gen(d[e0 + 1][0], A1, B1[e0 + 1]); h1gen(d[e0 + 1][1], A2, B1[e0 + 1]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
        } else
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) {
            const int fs = bt & 1;                  // fragment set of this batch; the next batch's goes into fs ^ 1
            // the NEXT batch's fragments: column blocks 2 bt + 2, 2 bt + 3 of this chunk, then 0, 1 of the next chunk
            const char* rn = (bt < 3) ? rb0 + (2 * bt + 2) * 2048 : rb1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const int t = i >> 1, nb = i & 1;       // product-major: consecutive MFMAs go to different accumulators
                    const int cbk = 2 * bt + nb;
                    const int n = bt * 24 + e * 6 + i;      // MFMA index in the chunk
                    if (!((FLAGS & 128) && t == 2))
                        acc[e][cbk] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, t == 2 ? alo[e] : ahi[e]), t == 0 ? blo[fs][nb] : bhi[fs][nb], acc[e][cbk], 0, 0, 0);
                    asm volatile("" : "+a"(acc[e][cbk]));
                    // conversions of the next chunk's operands: edge block ce from the gap behind its last MFMA (n = 77 + 6 ce)
                    // on, 8 gaps each (pair p: first part, then second part), wrapping into the next chunk's first 14 gaps -
                    // edge block ce is first read there at n = 6 ce
                    {
                        const int k = n >= 78 ? n - 78 : n + 18;
                        if ((FLAGS & 1) && k < 32) {
                            const int ce = k >> 3, jp = (k & 7) >> 1;
                            if ((k & 1) == 0) conv_a(d[ce][jp >> 1][2 * (jp & 1)], d[ce][jp >> 1][2 * (jp & 1) + 1], cph, ct0, ct1);
                            else {
                                conv_b(jp, cph, ct0, ct1, ahi[ce], alo[ce]);
                                asm volatile("" ::"v"(ahi[ce]), "v"(alo[ce]));
                            }
                        }
                    }
                    if ((FLAGS & 16) && e == 1) {           // the other set's last reader was the previous batch
                        if (i == 0) blo[fs ^ 1][0] = *(const h8*)(rn + (bo ^ 64));
                        if (i == 1) blo[fs ^ 1][1] = *(const h8*)(rn + 2048 + (bo ^ 64));
                        if (i == 2) bhi[fs ^ 1][0] = *(const h8*)(rn + bo);
                        if (i == 3) bhi[fs ^ 1][1] = *(const h8*)(rn + 2048 + bo);
                    }
                    if ((FLAGS & 4) && bt == 1 && i == 5) issue_w2(dchunk, dslot, e);
                    if ((FLAGS & 8) && bt == 1 && e == 0 && i == 1) A1 = *(const h8*)w1n;
                    if ((FLAGS & 8) && bt == 1 && e == 0 && i == 3) A2 = *(const h8*)(w1n + 256);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (bt == 1 && (FLAGS & 8)) {
                // H1 of the next chunk (single-buffered raw H1: its last reader, edge block 3's conversion, ran in the first
                // 14 gaps of this chunk; the first reader is 30 MFMAs on)
#pragma unroll
                for (int e1 = 0; e1 < 4; ++e1) { h1gen(d[e1][0], A1, B1[e1]); h1gen(d[e1][1], A2, B1[e1]); }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (FLAGS & 4) {
            if (LV >= 3) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");       // the ring pieces are retired, the four x_j DMA stay in flight
            else if (NS == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        }
        if (FLAGS & 2) __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        slot = slot1;
    }
    long t1 = clock64();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (FLAGS & 32) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nb = 0; nb < 8; ++nb) asm volatile("" : "+a"(Z[e][nb]));
    }
    float s = 0;
    for (int e = 0; e < 4; ++e)
        for (int nb = 0; nb < 8; ++nb)
            for (int r = 0; r < 4; ++r) s += acc[e][nb][r] + ((FLAGS & 32) ? Z[e][nb][r] : 0.f);
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = t1 - t0;
    if (s == 1234.5f) out[1] = 1;
}

// SHAPE 0: v_mfma_f32_32x32x16_f16, 1: v_mfma_f32_16x16x32_f16 (batch-major: the kernel up to the levelled K loop), 2: the same
// MFMAs in the levelled, half-chunk-major schedule, 3: levelled with four resident fragment sets, 4: 3 as a peeled chunk with its side
// loads, 5: 4 with the accumulator copies of the kernel's peeled chunks
template <int FLAGS, int NS, int SHAPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void kern(long* out, const char* gsrc, float seed, int iters) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (SHAPE == 0) body32<FLAGS, NS>(smem, out, gsrc, seed, iters);
    else if (SHAPE == 1) body16<FLAGS, NS, 0>(smem, out, gsrc, seed, iters);
    else if (SHAPE == 2) body16<FLAGS, NS, 1>(smem, out, gsrc, seed, iters);
    else if (SHAPE == 3) body16<FLAGS, NS, 2>(smem, out, gsrc, seed, iters);
    else if (SHAPE == 4) body16<FLAGS, NS, 3>(smem, out, gsrc, seed, iters);
    else body16<FLAGS, NS, 4>(smem, out, gsrc, seed, iters);
}

// Does the immediate offset of global_load_lds advance BOTH the global address and the LDS address?
__global__ void dma_offset_test(const unsigned* g, unsigned* out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (int i = threadIdx.x; i < 2048; i += 64) ((unsigned*)smem)[i] = 0xdeadbeefu;
    __syncthreads();
    const char* gp = (const char*)g + threadIdx.x * 16;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp, (__attribute__((address_space(3))) void*)smem, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp, (__attribute__((address_space(3))) void*)smem, 16, 1024, 0);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp, (__attribute__((address_space(3))) void*)smem, 16, 3072, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int i = threadIdx.x; i < 2048; i += 64) out[i] = ((unsigned*)smem)[i];
}

template <int FLAGS, int NS, int SHAPE = 0>
double run(long* d, const char* src, const char* what, int iters = 2048, double* cyc_out = nullptr) {
    const int lds = NS * TILE_B + 32768 + (SHAPE >= 4 ? 16384 : 0);      // SHAPE 4, 5: + 4 KiB of x_j rows per wave
    hipFuncSetAttribute((const void*)kern<FLAGS, NS, SHAPE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL((kern<FLAGS, NS, SHAPE>), dim3(256), dim3(256), lds, 0, d, src, 1.0f, 64);
    hipDeviceSynchronize();
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    hipEventRecord(a, 0);
    hipLaunchKernelGGL((kern<FLAGS, NS, SHAPE>), dim3(256), dim3(256), lds, 0, d, src, 1.0f, iters);
    hipEventRecord(b, 0);
    hipEventSynchronize(b);
    float ms = 0;
    hipEventElapsedTime(&ms, a, b);
    hipEventDestroy(a); hipEventDestroy(b);
    long hcyc;
    hipMemcpy(&hcyc, d, 8, hipMemcpyDeviceToHost);
    // MFMA work in units of one 32x32x16 (= two 16x16x32: the same FLOP and the same 32 matrix-pipe cycles)
    const int nm = ((FLAGS & 128) ? 32 : 48) + ((FLAGS & 8) ? 4 : 0);
    const double tf = 256.0 * 4 * iters * nm * 32768.0 / (ms * 1e-3) / 1e12;
    // shader clock over the run: the K loop's clock64() cycles of one wave / the kernel's event time (prologue / epilogue of
    // the kernel are < 1 % of 2048 iterations); matrix pipe occupancy = MFMA cycles issued / cycles elapsed
    const double ghz = (double)hcyc / (ms * 1e-3) / 1e9;
    printf("%s NS %d flags %3d %-46s: %6.0f cycles/chunk (MFMA %d = %4.1f %% of the cycles)  clock %.3f GHz  %7.1f TFLOP/s  %.2f ms  err=%s\n",
           SHAPE == 5 ? "16x16 cp" : SHAPE == 4 ? "16x16 sl" : SHAPE == 3 ? "16x16 rf" : SHAPE == 2 ? "16x16 lv" : SHAPE ? "16x16x32" : "32x32x16", NS, FLAGS, what,
           (double)hcyc / iters, nm * 32, 100.0 * nm * 32 * iters / (double)hcyc, ghz, tf, ms, hipGetErrorString(hipGetLastError()));
    if (cyc_out) *cyc_out = (double)hcyc / iters;
    return tf;
}

int main(int argc, char** argv) {
    const bool only_copy = argc > 1 && !strcmp(argv[1], "copy");      // `kloop_model_v6 copy`: the copy A/B alone
    const int REPS = 4, LONG = 32768;
    double least = 1e9;
    long* d; char* src;
    hipMalloc(&d, 64);
    const size_t nsrc = (size_t)8 * 32 * TILE_B;
    hipMalloc(&src, nsrc);
    {   // random f16 bit patterns in a sane range (power draw depends on the data)
        unsigned short* hsrc = (unsigned short*)malloc(nsrc);
        unsigned s = 12345u;
        for (size_t i = 0; i < nsrc / 2; ++i) { s = s * 1664525u + 1013904223u; hsrc[i] = (unsigned short)(0x3000u + ((s >> 16) & 0x0fffu) + ((s >> 3) & 0x8000u)); }
        hipMemcpy(src, hsrc, nsrc, hipMemcpyHostToDevice);
        free(hsrc);
    }
    {
        unsigned *g, *o, hg[2048], ho[2048];
        for (int i = 0; i < 2048; ++i) hg[i] = i;
        hipMalloc(&g, 8192); hipMalloc(&o, 8192);
        hipMemcpy(g, hg, 8192, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(dma_offset_test, dim3(1), dim3(64), 8192, 0, g, o);
        hipMemcpy(ho, o, 8192, hipMemcpyDeviceToHost);
        int ok = 1;
        for (int i = 0; i < 2048; ++i) {
            const int piece = i / 256;
            const unsigned want = (piece == 0 || piece == 1 || piece == 3) ? (unsigned)i : 0xdeadbeefu;
            if (ho[i] != want) { if (ok) printf("dma offset test: word %d = %u, expected %u\n", i, ho[i], want); ok = 0; }
        }
        printf("dma immediate offset advances global AND lds address: %s\n", ok ? "YES" : "NO");
    }
    if (!only_copy) {
    run<0, 3>(d, src, "48 MFMA only");
    run<16, 3>(d, src, "+ 16 W2 fragment reads");
    run<16 | 8, 3>(d, src, "+ H1 (4 MFMA, 2 LDS reads)");
    run<16 | 8 | 1, 3>(d, src, "+ conversions");
    run<16 | 8 | 1 | 32, 3>(d, src, "+ 128 live Z registers");
    run<16 | 8 | 1 | 32 | 2, 3>(d, src, "+ s_barrier per chunk");
    run<16 | 8 | 1 | 32 | 2 | 4, 3>(d, src, "+ DMA ring, wait per chunk (FULL, 3 slots)");
    run<16 | 8 | 1 | 32 | 4, 3>(d, src, "DMA, no barrier (racy, timing only)");
    run<16 | 8 | 1 | 32 | 2 | 4, 4>(d, src, "FULL, 4 slots (DMA two chunks ahead)");
    run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3>(d, src, "FULL, 3 slots, H1 MFMA into VGPRs (asm)");
    run<64 | 16 | 8 | 1 | 32 | 2 | 4, 4>(d, src, "FULL, 4 slots, H1 MFMA into VGPRs (asm)");
    run<128, 3>(d, src, "32 MFMA only (2 of 3 split products)");
    run<128 | 64 | 16 | 8 | 1 | 32 | 2 | 4, 3>(d, src, "FULL, 3 slots, asm H1, 2 of 3 split products");

    // the same ladder on v_mfma_f32_16x16x32_f16
    run<0, 3, 1>(d, src, "96 MFMA only");
    run<16, 3, 1>(d, src, "+ 16 W2 fragment reads");
    run<16 | 8, 3, 1>(d, src, "+ H1 (8 MFMA, 2 LDS reads)");
    run<16 | 8 | 1, 3, 1>(d, src, "+ conversions");
    run<16 | 8 | 1 | 32, 3, 1>(d, src, "+ 128 live Z registers");
    run<16 | 8 | 1 | 32 | 2, 3, 1>(d, src, "+ s_barrier per chunk");
    run<16 | 8 | 1 | 32 | 2 | 4, 3, 1>(d, src, "+ DMA ring, wait per chunk (FULL, 3 slots)");
    run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3, 1>(d, src, "FULL, 3 slots, H1 MFMA into VGPRs (asm)");

    // Shape A/B: bare stream and full model (the production configuration: 3 slots, asm H1) of both shapes, alternating,
    // at 16 x the iterations (launches of tens of ms, so the clock the chip settles at is the one measured)
    double worst_bare = 1e9, worst_full = 1e9;
    for (int r = 0; r < REPS; ++r) {
        printf("shape A/B repetition %d\n", r);
        const double b32 = run<0, 3, 0>(d, src, "bare stream", LONG);
        const double b16 = run<0, 3, 1>(d, src, "bare stream", LONG);
        const double f32_ = run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3, 0>(d, src, "FULL model", LONG);
        const double f16_ = run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3, 1>(d, src, "FULL model", LONG);
        printf("  16x16x32 / 32x32x16 FLOP/s: bare %.4f  full %.4f\n", b16 / b32, f16_ / f32_);
        if (b16 / b32 < worst_bare) worst_bare = b16 / b32;
        if (f16_ / f32_ < worst_full) worst_full = f16_ / f32_;
    }
    printf("shape A/B lowest ratio over %d repetitions: bare %.4f  full %.4f\n", REPS, worst_bare, worst_full);

    // Schedule A/B on 16x16x32: the ladder of the levelled schedule, then the full model batch-major against levelled,
    // alternating, four repetitions.  The gate for a kernel change: levelled lower by >= 100 cycles per chunk in EVERY repetition
    run<16, 3, 2>(d, src, "+ 32 W2 fragment reads");
    run<16 | 8, 3, 2>(d, src, "+ H1 (8 MFMA, 2 LDS reads)");
    run<64 | 16 | 8 | 1, 3, 2>(d, src, "+ conversions, one per gap (asm H1)");
    run<64 | 16 | 8 | 1 | 32, 3, 2>(d, src, "+ 128 live Z registers");
    run<64 | 16 | 8 | 1 | 32 | 2, 3, 2>(d, src, "+ s_barrier per chunk");
    run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3, 2>(d, src, "+ DMA ring, wait per chunk (FULL)");
    least = 1e9;
    for (int r = 0; r < REPS; ++r) {
        printf("schedule A/B repetition %d\n", r);
        double ca = 0, cb = 0;
        const double fa = run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3, 1>(d, src, "FULL model, batch-major", LONG, &ca);
        const double fb = run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3, 2>(d, src, "FULL model, levelled", LONG, &cb);
        printf("  cycles per chunk saved %.0f   levelled / batch-major FLOP/s %.4f\n", ca - cb, fb / fa);
        if (ca - cb < least) least = ca - cb;
    }
    printf("schedule A/B least saving over %d repetitions: %.0f cycles per chunk (gate: 100)\n", REPS, least);

    // Fragment A/B: the levelled schedule with two fragment sets (32 reads per chunk) against four resident sets (16 reads), first
    // without the DMA ring, then the full model, alternating, four repetitions.  The gate for a kernel change: a saving in EVERY
    // repetition (the model repeats to within a cycle or two)
    run<64 | 16 | 8 | 1 | 32 | 2, 3, 3>(d, src, "16 W2 fragment reads, no DMA ring");
    run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3, 3>(d, src, "+ DMA ring, wait per chunk (FULL)");
    least = 1e9;
    for (int r = 0; r < REPS; ++r) {
        printf("fragment A/B repetition %d\n", r);
        double ca = 0, cb = 0;
        const double fa = run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3, 2>(d, src, "FULL model, levelled, 32 reads", LONG, &ca);
        const double fb = run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3, 3>(d, src, "FULL model, levelled, 16 reads", LONG, &cb);
        printf("  cycles per chunk saved %.1f   resident / re-read FLOP/s %.4f\n", ca - cb, fb / fa);
        if (ca - cb < least) least = ca - cb;
    }
    printf("fragment A/B least saving over %d repetitions: %.1f cycles per chunk (gate: > 0 in every repetition)\n", REPS, least);
    }

    // Copy A/B: a peeled chunk of the image variant (resident sets + the side loads of chunks 3-5) with tied accumulators against the
    // same chunk with the accumulator copies hipcc places there, and the steady chunk next to them: what the side loads cost on their
    // own (SHAPE 4 - SHAPE 3) and what the copies cost (SHAPE 5 - SHAPE 4).  The gate for tied product MFMAs in the kernel: a saving
    // in EVERY repetition
    least = 1e9;
    for (int r = 0; r < REPS; ++r) {
        printf("copy A/B repetition %d\n", r);
        double c3 = 0, ca = 0, cb = 0;
        run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3, 3>(d, src, "FULL model, steady chunk", LONG, &c3);
        const double fa = run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3, 5>(d, src, "FULL model, peeled chunk, 32 copies", LONG, &ca);
        const double fb = run<64 | 16 | 8 | 1 | 32 | 2 | 4, 3, 4>(d, src, "FULL model, peeled chunk, tied", LONG, &cb);
        printf("  cycles per chunk: side loads %.1f, copies %.1f   tied / copies FLOP/s %.4f\n", cb - c3, ca - cb, fb / fa);
        if (ca - cb < least) least = ca - cb;
    }
    printf("copy A/B least saving over %d repetitions: %.1f cycles per chunk (gate: > 0 in every repetition)\n", REPS, least);
    return 0;
}
