// IQ4_NL / IQ4_XS members of the generation-2 prompt mat-mul family (mmq2_kernels.hip has the structure's description and the k-quant / Q4_0 members; the
// launch arguments, the activation staging and the result store are the family's own: mmq2_common.hpp).
//
// Both formats store a nibble per weight that indexes the 16-entry int8 codebook, so after the lookup the weight IS an int8 MFMA operand: no offset (Q4_0's q - 8 is
// gone), no min term (Q4_K's two digit-plane MFMAs are gone, its staged per-32 sums go unread).  The lookup is the new cost -- iq4_lut4: seven vector operations per
// four weights, 16 dwords per lane and super-block -- and it is paid ONCE per 256 weights and row tile: the eight B operands (32 VGPRs) it fills are reused for every
// token tile of the chunk, up to 32 TT tokens.
//   * a unit (16 bytes of the main plane) = 32 consecutive weights, low nibbles = elements 0..15, high nibbles = 16..31 (IQ4_NL: a block, IQ4_XS: sub-block ib), so
//     lane half hh takes the low / high nibbles of unit b and the A fragment is chunk 2 b + hh of the token's staged row: one K = 32 MFMA per 32 weights;
//   * IQ4_XS (Q8_K rows, Mmq2Stage): one integer multiply-add per (row, token, sub-block) with ls - 32 -- a per-lane scalar, the lane owns the weight row; |ls - 32| <= 32
//     and |sum kv a| < 2^19: the 24-bit multiplier is exact -- then ONE fp32 d_w * d_a per super-block: ggml's vec_dot_iq4_xs_q8_K;
//   * IQ4_NL (Q8_0 rows, Mmq2Stage80): per block acc = fma(d_w * d_a, (float)isum, acc) as k_mmq2_q40 and Tr<GT_IQ4_NL>::dot do it: ggml's vec_dot_iq4_nl_q8_0.
// Without a K split every output adds its per-block terms in block order.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 149 .. 210 VGPRs, no scratch -- the table at launch_mmq2_iq4.
#include "mmq2_common.hpp"
#include <type_traits>

namespace mg4 {

template <bool XS, int TT, int WPB = 4>
__global__ __launch_bounds__(64 * WPB, 2) void k_mmq2_iq4(const Mmq2Args a, const ActQ A) {
    using S = std::conditional_t<XS, Mmq2Stage<TT>, Mmq2Stage80<TT>>;
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem_mmq2[];   // [2 activation stages][4 waves x 4 KiB weight transpose scratch]
    const int lane = threadIdx.x & 63, hh = lane >> 5, l31 = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = blockIdx.x / a.groups_each, g = blockIdx.x - m * a.groups_each;
    const QWeight W = a.w[m];
    const int K = W.cols, U = K / 32, NSB = K / 256, N = a.N;
    const int r0 = (g * WPB + wv) * 32;
    const int row = min(r0 + l31, W.rows - 1);
    const int tile0 = blockIdx.y * a.tiles_per_chunk, my_tiles = min(TT, a.n_tiles - tile0), t0 = tile0 * 32;
    const int sb0 = blockIdx.z * a.sb_per_split, sb1 = min(NSB, sb0 + a.sb_per_split);
    unsigned char *scratch = smem_mmq2 + 2 * S::BYTES + wv * 4096;
    const int n_q8 = (min(N - t0, 32 * TT) + 3) / 4;             // q8 staging instructions that carry live tokens (single-wave form)

    typedef float v16f_t __attribute__((ext_vector_type(16)));
    v16f_t acc[TT];
#pragma unroll
    for (int tt = 0; tt < TT; tt++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[tt][r] = 0.0f;

    // coalesced weight requests (see k_mmq2_q45k): main plane 8 rows x 128 B per instruction; scale plane: 16 bytes per row and super-block in either format
    // (IQ4_NL: the 8 blocks' fp16 d; IQ4_XS: {d, -, 8 x int8 ls - 32})
    struct Raw { v4i q[4]; v4i h; };
    const unsigned char *wq[4];
#pragma unroll
    for (int n = 0; n < 4; n++) wq[n] = W.qs + ((size_t)min(r0 + 8 * n + (lane >> 3), W.rows - 1) * U + (lane & 7)) * 16;
    const unsigned char *wh = W.sc + (size_t)row * NSB * 16;
    auto fetch = [&](int sb, Raw &w) {
#pragma unroll
        for (int n = 0; n < 4; n++) w.q[n] = ldg16(wq[n] + (size_t)sb * 128);
        w.h = ldg16(wh + (size_t)sb * 16);
    };
    unsigned sw_addr[4], sr_addr[8], a_addr[8];
#pragma unroll
    for (int n = 0; n < 4; n++) sw_addr[n] = (unsigned)((8 * n + (lane >> 3)) * 128 + (((lane & 7) ^ ((4 * n + (lane >> 4)) & 7)) << 4));
#pragma unroll
    for (int b = 0; b < 8; b++) sr_addr[b] = (unsigned)(l31 * 128 + ((b ^ ((l31 >> 1) & 7)) << 4));     // both lane halves read unit b of their row (hh selects the nibble)
    const int v = hh ^ (lane & 15);
#pragma unroll
    for (int b = 0; b < 8; b++) a_addr[b] = (unsigned)(l31 * 256 + (((2 * b) ^ v) << 4));                // elements 32 b + 16 hh .. + 15 of token l31
    const unsigned sc_addr = (unsigned)(S::Q8 + (XS ? Mmq2Stage<TT>::BS : 0) + 16 * hh);                 // the activation scales of tokens 4 hh .. 4 hh + 3 (+ 8 q4)

    unsigned tokoff[S::TTP / 2];                                                                         // IQ4_NL: this lane's row offsets into A.d0 (mmq2_stage_load80)
#pragma unroll
    for (int j = 0; j < S::TTP / 2; j++) tokoff[j] = (unsigned)min(t0 + 64 * j + lane, N - 1) * (unsigned)(K / 32);
    auto stage = [&](int sb, unsigned char *st) {
        if constexpr (XS) mmq2_stage_load<TT, WPB>(A, K, NSB, N, t0, sb, st, wv, lane, n_q8);
        else mmq2_stage_load80<TT, WPB>(A, K, N, t0, sb, st, wv, lane, tokoff, n_q8);
    };
    Raw raw;
    fetch(sb0, raw);
    stage(sb0, smem_mmq2);
    for (int sb = sb0; sb < sb1; sb++) {
        const int buf = (sb - sb0) & 1;
        unsigned char *st = smem_mmq2 + buf * S::BYTES;
        __syncthreads();                                           // own DMA + weight loads done, then everybody's
        // ---- this super-block's weights: transpose through LDS, then nibble -> codebook int8, straight into the eight B operands
#pragma unroll
        for (int n = 0; n < 4; n++) *reinterpret_cast<v4i *>(scratch + sw_addr[n]) = raw.q[n];
        v4i wb[8];
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const v4i q = *reinterpret_cast<const v4i *>(scratch + sr_addr[b]);
#pragma unroll
            for (int w = 0; w < 4; w++) wb[b][w] = iq4_lut4(hh ? ((unsigned)q[w] >> 4) & 0x0F0F0F0Fu : (unsigned)q[w] & 0x0F0F0F0Fu);
        }
        float dw[XS ? 1 : 8]; int ls[XS ? 8 : 1];
        if constexpr (XS) {
            dw[0] = h2f_b((unsigned)raw.h[0] & 0xFFFF);
#pragma unroll
            for (int b = 0; b < 8; b++) ls[b] = (int)(signed char)((unsigned)raw.h[2 + (b >> 2)] >> (8 * (b & 3)));
        } else {
#pragma unroll
            for (int b = 0; b < 8; b++) dw[b] = h2f_b(((unsigned)raw.h[b >> 1] >> (16 * (b & 1))) & 0xFFFF);
        }
        __builtin_amdgcn_sched_barrier(0);                         // the raw registers are dead from here: the next super-block's loads reuse them
        {
            const int sbn = min(sb + 1, sb1 - 1);
            fetch(sbn, raw);
            stage(sbn, smem_mmq2 + (buf ^ 1) * S::BYTES);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- token tiles: the MFMA of unit b + 1 is issued before the vector arithmetic that consumes unit b's result (two result sets, as in the family's other members)
#pragma unroll
        for (int tt = 0; tt < TT; tt++) {
            if (tt < my_tiles) {
                const unsigned char *sq = st + tt * 8192;
                v16i D[2];
                v16i isum = zero16();
#define MMQ2_ISSUE_IQ(b, k) { const v4i af_ = *reinterpret_cast<const v4i *>(sq + a_addr[b]); D[k] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af_, wb[b], zero16(), 0, 0, 0); }
#define MMQ2_USE_IQ(b, k) { if constexpr (XS) {                                                                                                                    \
                                _Pragma("unroll") for (int r = 0; r < 16; r++) isum[r] = __mul24(D[k][r], ls[b]) + isum[r];                                           \
                                asm volatile("" : "+v"(isum));     /* one v_mad_i32_i24 per element, kept between the MFMAs */                                     \
                            } else {                                                                                                                               \
                                _Pragma("unroll") for (int q4 = 0; q4 < 4; q4++) {                                                                                 \
                                    const v4f da = *reinterpret_cast<const v4f *>(st + sc_addr + ((b) * S::TTP * 32 + tt * 32 + 8 * q4) * 4);                         \
                                    _Pragma("unroll") for (int e = 0; e < 4; e++) { const int r = 4 * q4 + e; acc[tt][r] = fmaf(dw[XS ? 0 : (b)] * da[e], (float)D[k][r], acc[tt][r]); } } \
                                asm volatile("" : "+v"(acc[tt]));  /* keeps the block's scale arithmetic here (k_mmq2_q40) */                                      \
                            } }
                MMQ2_ISSUE_IQ(0, 0)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE_IQ(1, 1) MMQ2_USE_IQ(0, 0)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE_IQ(2, 0) MMQ2_USE_IQ(1, 1)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE_IQ(3, 1) MMQ2_USE_IQ(2, 0)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE_IQ(4, 0) MMQ2_USE_IQ(3, 1)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE_IQ(5, 1) MMQ2_USE_IQ(4, 0)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE_IQ(6, 0) MMQ2_USE_IQ(5, 1)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE_IQ(7, 1) MMQ2_USE_IQ(6, 0)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_USE_IQ(7, 1)
                __builtin_amdgcn_sched_barrier(0);
#undef MMQ2_ISSUE_IQ
#undef MMQ2_USE_IQ
                if constexpr (XS) {
#pragma unroll
                    for (int q4 = 0; q4 < 4; q4++) {
                        const v4f da = *reinterpret_cast<const v4f *>(st + sc_addr + tt * 128 + q4 * 32);   // tokens 8 q4 + 4 hh + 0..3 = accumulator registers 4 q4 .. 4 q4 + 3
#pragma unroll
                        for (int e = 0; e < 4; e++) { const int r = 4 * q4 + e; acc[tt][r] = fmaf(dw[0] * da[e], (float)isum[r], acc[tt][r]); }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    float accf[TT][16];
#pragma unroll
    for (int tt = 0; tt < TT; tt++)
#pragma unroll
        for (int r = 0; r < 16; r++) accf[tt][r] = acc[tt][r];
    mmq2_store<TT>(accf, a, m, r0 + l31, W.rows, t0, my_tiles, hh);
}

template <bool XS, int TT>
static void launch_iq4_tt(dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A) {
    using S = std::conditional_t<XS, Mmq2Stage<TT>, Mmq2Stage80<TT>>;
    static bool attr = false;
    if (!attr) { HIP_IGNORE(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mmq2_iq4<XS, TT>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024)); attr = true; }
    hipLaunchKernelGGL((k_mmq2_iq4<XS, TT>), grid, dim3(256), (size_t)(2 * S::BYTES + 16384), s, a, A);
}
// VGPRs / scratch bytes per kernel (budget: <= 256 VGPRs, two workgroups per CU):        TT = 1        2        3
//                                                                         IQ4_NL      149 / 0   174 / 0   196 / 0
//                                                                         IQ4_XS      154 / 0   186 / 0   210 / 0
void launch_mmq2_iq4(int type, dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A) {
    const bool xs = type == GT_IQ4_XS;
    switch (a.tiles_per_chunk) {
    case 1: if (xs) launch_iq4_tt<true, 1>(grid, s, a, A); else launch_iq4_tt<false, 1>(grid, s, a, A); break;
    case 2: if (xs) launch_iq4_tt<true, 2>(grid, s, a, A); else launch_iq4_tt<false, 2>(grid, s, a, A); break;
    case 3: if (xs) launch_iq4_tt<true, 3>(grid, s, a, A); else launch_iq4_tt<false, 3>(grid, s, a, A); break;
    default: throw HipError{hipErrorInvalidValue, "mmq2: bad chunking", __FILE__, __LINE__};
    }
}

}  // namespace mg4
