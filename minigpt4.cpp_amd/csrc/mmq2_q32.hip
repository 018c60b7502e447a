// Q8_0 / Q5_0 / Q5_1 / Q4_1 members of the generation-2 prompt mat-mul family (mmq2_kernels.hip has the structure's description and the k-quant / Q4_0 members; the
// launch arguments, the activation staging and the result store are the family's own: mmq2_common.hpp).  Until these, N >= 5 rows against a file of one of the four
// formats ran on k_mul_mat<T, 2, 4>: v_dot4 on the vector ALU and one pass over the weights per FOUR rows.
//
// One kernel template, k_mmq2_q32<T, TT>, with k_mmq2_q40's skeleton (4 waves x 32 weight rows x TT <= 3 token tiles x one K range; Q8_0 activation rows by LDS-DMA,
// source-side swizzled, double buffered; weights read coalesced and transposed through the wave's 4 KiB LDS scratch; one barrier per 256-weight super-chunk; lane = weight
// row, so block scales are per-lane scalars; one K = 32 v_mfma_i32_32x32x32_i8 per block).  What each format changes, and why:
//   * Q8_0: the weights ARE int8 MFMA operands: no unpack at all, lane half hh's B operand of block b is bytes 16 hh .. 16 hh + 15 of the block as stored, against chunk
//     2 b + hh of the token's staged row.  A super-chunk of a row is 256 bytes, twice what the scratch holds per row, so it goes through the SAME scratch as two halves of
//     four blocks (write half 0, read its four operands, write half 1, read: LDS operations of one wave execute in order, no barrier between them).  Widening the scratch
//     to 8 KiB per wave was the other form: 88 KiB per workgroup at TT = 3, two workgroups = 176 KiB > the CU's 160 KiB, i.e. one workgroup per CU exactly where the chunk
//     is largest.  As built: 2 x 28672 (stages) + 16384 (scratch) = 73728 bytes = 72 KiB per workgroup at TT = 3, like k_mmq2_q40.  The weight requests keep Q4_0's
//     coalescing (instruction n of a half: rows 8 n .. 8 n + 7 x 128 contiguous bytes); there are eight of them per super-chunk instead of four.
//   * Q5_0: Q4_0's main plane + the pre-transposed high-bit word P of the block (qh plane, pack_hb1: MG4_Q5_DOT8's shifts).  Both lane halves read unit b; the half selects
//     the nibble (shift 0 / 4) and its high bits ((hh ? P : P << 4) >> k, one shift per dword: P << 4 moves the low elements' bits to where the high elements' sit).  nibble | bit,
//     then - 16 per byte with the borrow-free subtraction k_mmq2_q40 uses for - 8: the operand is the int8 weight, no per-32 sum correction.  A lane keeps the 8 words of
//     its row and super-chunk (32 bytes, two requests; the other lane half requests the same bytes: one cache line).
//   * Q4_1 / Q5_1: quants stay unsigned (0..15, 0..31 fit int8), scale plane {d, m} (two requests of 16 bytes per row and super-chunk), activations scaled by A.d1, and
//     a second term per block, m_w * s_a with s_a = A.s1.  The stage carries a second fp32 plane laid out like the first ([8 blocks][TTP * 32 tokens]): + 4096 bytes at
//     TT = 3 -> 2 x 32768 + 16384 = 81920 bytes = 80 KiB per workgroup, two workgroups = the CU's 160 KiB exactly (TT = 1, 2: 40 / 56 KiB).
// Per block and output: acc = fma(d_w * d_a, (float)isum, acc), for the _1 formats then acc = fma(m_w, s_a, acc): the products of Tr<T>::terms.  Without a K split every
// output adds its blocks' terms in block order, so it equals k_mul_mat_ref's value bit for bit (parity mode's prompt rows; tests/test_gpu_mmq2_q32.py).
// Each block's conversion and fma's stay next to its MFMA (the asm pin on the accumulators and the sched_barrier pattern of k_mmq2_q40).
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): the table at launch_mmq2_q32; no member uses scratch memory.
#include "mmq2_common.hpp"
#include <type_traits>

namespace mg4 {

template <int T, int TT>
__global__ __launch_bounds__(256, 2) void k_mmq2_q32(const Mmq2Args a, const ActQ A) {
    constexpr bool Q8 = T == GT_Q8_0, HB = T == GT_Q5_0 || T == GT_Q5_1, M1 = T == GT_Q4_1 || T == GT_Q5_1;
    using S = Mmq2Stage80<TT>;
    constexpr int STAGE = S::BYTES + (M1 ? S::DS : 0);          // _1: the s1 plane behind the d1 plane
    constexpr int QB = Q8 ? 32 : 16;                            // main-plane bytes per block
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem_mmq2[];   // [2 activation stages][4 waves x 4 KiB weight transpose scratch]
    const int lane = threadIdx.x & 63, hh = lane >> 5, l31 = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = blockIdx.x / a.groups_each, g = blockIdx.x - m * a.groups_each;
    const QWeight W = a.w[m];
    const int K = W.cols, U = K / 32, NSB = K / 256, N = a.N;
    const int r0 = (g * 4 + wv) * 32;
    const int row = min(r0 + l31, W.rows - 1);
    const int tile0 = blockIdx.y * a.tiles_per_chunk, my_tiles = min(TT, a.n_tiles - tile0), t0 = tile0 * 32;
    const int sb0 = blockIdx.z * a.sb_per_split, sb1 = min(NSB, sb0 + a.sb_per_split);
    unsigned char *scratch = smem_mmq2 + 2 * STAGE + wv * 4096;

    typedef float v16f_t __attribute__((ext_vector_type(16)));
    v16f_t acc[TT];
#pragma unroll
    for (int tt = 0; tt < TT; tt++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[tt][r] = 0.0f;

    // coalesced weight requests (see k_mmq2_q45k): main plane 8 rows x 128 contiguous bytes per instruction (Q8_0: per half); per row the super-chunk's 8 high-bit words
    // (32 bytes) and its 8 scales (fp16 d: 16 bytes; {d, m}: 32 bytes)
    struct Raw { v4i q[Q8 ? 8 : 4]; v4i p[HB ? 2 : 1]; v4i h[M1 ? 2 : 1]; };
    const unsigned char *wq[4];
#pragma unroll
    for (int n = 0; n < 4; n++) wq[n] = W.qs + ((size_t)min(r0 + 8 * n + (lane >> 3), W.rows - 1) * U * QB + (lane & 7) * 16);
    const unsigned char *wp = HB ? W.qh + (size_t)row * U * 4 : nullptr, *wh = W.sc + (size_t)row * U * (M1 ? 4 : 2);
    auto fetch = [&](int sb, Raw &w) {
#pragma unroll
        for (int n = 0; n < 4; n++) {
            w.q[n] = ldg16(wq[n] + (size_t)sb * (8 * QB));
            if constexpr (Q8) w.q[4 + n] = ldg16(wq[n] + (size_t)sb * 256 + 128);
        }
        if constexpr (HB) { w.p[0] = ldg16(wp + (size_t)sb * 32); w.p[1] = ldg16(wp + (size_t)sb * 32 + 16); }
        w.h[0] = ldg16(wh + (size_t)sb * (M1 ? 32 : 16));
        if constexpr (M1) w.h[1] = ldg16(wh + (size_t)sb * 32 + 16);
    };
    unsigned sw_addr[4], sr_addr[Q8 ? 4 : 8], a_addr[8];
#pragma unroll
    for (int n = 0; n < 4; n++) sw_addr[n] = (unsigned)((8 * n + (lane >> 3)) * 128 + (((lane & 7) ^ ((4 * n + (lane >> 4)) & 7)) << 4));
    if constexpr (Q8) {
#pragma unroll
        for (int b = 0; b < 4; b++) sr_addr[b] = (unsigned)(l31 * 128 + (((2 * b + hh) ^ ((l31 >> 1) & 7)) << 4));   // unit 2 b + hh of the half: bytes 16 hh .. of its block b
    } else {
#pragma unroll
        for (int b = 0; b < 8; b++) sr_addr[b] = (unsigned)(l31 * 128 + ((b ^ ((l31 >> 1) & 7)) << 4));              // both lane halves read unit b of their row (hh selects the nibble)
    }
    const int v = hh ^ (lane & 15);
#pragma unroll
    for (int b = 0; b < 8; b++) a_addr[b] = (unsigned)(l31 * 256 + (((2 * b) ^ v) << 4));                // elements 32 b + 16 hh .. + 15 of token l31
    const unsigned ds_addr = (unsigned)(S::Q8 + 16 * hh);
    const int nsh = 4 * hh, psh = 4 - 4 * hh;                                                            // nibble shift; high-bit word: low elements' bits up to the high elements' places

    unsigned tokoff[S::TTP / 2];
#pragma unroll
    for (int j = 0; j < S::TTP / 2; j++) tokoff[j] = (unsigned)min(t0 + 64 * j + lane, N - 1) * (unsigned)(K / 32);
    ActQ A8 = A;
    if constexpr (M1) A8.d0 = A.d1;                              // the family's Q8_0 stage with the Q8_1 scale as its scale plane
    auto stage = [&](int sb, unsigned char *st) {
        mmq2_stage_load80<TT, 4>(A8, K, N, t0, sb, st, wv, lane, tokoff, 8 * TT);
        if constexpr (M1) {                                      // s1 like the first plane: wave wv takes blocks wv and wv + 4, instruction j tokens 64 j + lane
#pragma unroll
            for (int j = 0; j < S::TTP / 2; j++) {
                const float *pj = A.s1 + (size_t)tokoff[j] + (size_t)sb * 8 + wv;
                dma4(pj, st + S::BYTES + (wv * S::TTP * 32 + 64 * j) * 4);
                dma4(pj + 4, st + S::BYTES + ((wv + 4) * S::TTP * 32 + 64 * j) * 4);
            }
        }
    };
    Raw raw;
    fetch(sb0, raw);
    stage(sb0, smem_mmq2);
    for (int sb = sb0; sb < sb1; sb++) {
        const int buf = (sb - sb0) & 1;
        unsigned char *st = smem_mmq2 + buf * STAGE;
        __syncthreads();                                           // own DMA + weight loads done, then everybody's
        // ---- this super-chunk's weights: transpose through LDS, straight into the eight B operands
        v4i wb[8];
#pragma unroll
        for (int n = 0; n < 4; n++) *reinterpret_cast<v4i *>(scratch + sw_addr[n]) = raw.q[n];
        if constexpr (Q8) {
#pragma unroll
            for (int b = 0; b < 4; b++) wb[b] = *reinterpret_cast<const v4i *>(scratch + sr_addr[b]);
#pragma unroll
            for (int n = 0; n < 4; n++) *reinterpret_cast<v4i *>(scratch + sw_addr[n]) = raw.q[4 + n];
#pragma unroll
            for (int b = 0; b < 4; b++) wb[4 + b] = *reinterpret_cast<const v4i *>(scratch + sr_addr[b]);
        } else {
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const v4i q = *reinterpret_cast<const v4i *>(scratch + sr_addr[b]);
                const unsigned P = HB ? (unsigned)raw.p[b >> 2][b & 3] << psh : 0u;
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    unsigned x = ((unsigned)q[w] >> nsh) & 0x0F0F0F0Fu;
                    if constexpr (HB) x |= (P >> w) & 0x10101010u;
                    if constexpr (T == GT_Q5_0) x = ((x | 0x80808080u) - 0x10101010u) ^ 0x80808080u;   // per byte x - 16 as int8: bit 7 set keeps the subtraction from borrowing across bytes
                    wb[b][w] = (int)x;
                }
            }
        }
        float dw[8], mw[M1 ? 8 : 1];
#pragma unroll
        for (int b = 0; b < 8; b++) {
            if constexpr (M1) { const unsigned dm = (unsigned)raw.h[b >> 2][b & 3]; dw[b] = h2f_b(dm & 0xFFFF); mw[b] = h2f_b(dm >> 16); }
            else dw[b] = h2f_b(((unsigned)raw.h[0][b >> 1] >> (16 * (b & 1))) & 0xFFFF);
        }
        __builtin_amdgcn_sched_barrier(0);                         // the raw registers are dead from here: the next super-chunk's loads reuse them
        {
            const int sbn = min(sb + 1, sb1 - 1);
            fetch(sbn, raw);
            stage(sbn, smem_mmq2 + (buf ^ 1) * STAGE);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- token tiles: the MFMA of block b + 1 is issued before the vector arithmetic that consumes block b's result (two result sets, as in the family's other members)
        auto tile = [&](auto ttc) __attribute__((always_inline)) {
            constexpr int tt = decltype(ttc)::value;
            if (tt < my_tiles) {
                const unsigned char *sq = st + tt * 8192;
                v16i D[2];
#define MMQ2_ISSUE32(b, k) { const v4i af_ = *reinterpret_cast<const v4i *>(sq + a_addr[b]); D[k] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af_, wb[b], zero16(), 0, 0, 0); }
#define MMQ2_SCALE32(b, k) { _Pragma("unroll") for (int q4 = 0; q4 < 4; q4++) {                                                                                   \
                               const unsigned char *sp_ = st + ds_addr + ((b) * S::TTP * 32 + tt * 32 + 8 * q4) * 4;   /* tokens 8 q4 + 4 hh + 0..3 = registers 4 q4 .. 4 q4 + 3 */ \
                               const v4f da = *reinterpret_cast<const v4f *>(sp_);                                                                                 \
                               v4f sa; if constexpr (M1) sa = *reinterpret_cast<const v4f *>(sp_ + S::DS);                                                         \
                               _Pragma("unroll") for (int e = 0; e < 4; e++) { const int r = 4 * q4 + e;                                                           \
                                   acc[tt][r] = fmaf(dw[b] * da[e], (float)D[k][r], acc[tt][r]);                                                                   \
                                   if constexpr (M1) acc[tt][r] = fmaf(mw[b], sa[e], acc[tt][r]); } }                                                              \
                             asm volatile("" : "+v"(acc[tt])); }   /* keeps the block's scale arithmetic here (k_mmq2_q40) */
                MMQ2_ISSUE32(0, 0)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE32(1, 1) MMQ2_SCALE32(0, 0)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE32(2, 0) MMQ2_SCALE32(1, 1)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE32(3, 1) MMQ2_SCALE32(2, 0)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE32(4, 0) MMQ2_SCALE32(3, 1)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE32(5, 1) MMQ2_SCALE32(4, 0)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE32(6, 0) MMQ2_SCALE32(5, 1)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_ISSUE32(7, 1) MMQ2_SCALE32(6, 0)
                __builtin_amdgcn_sched_barrier(0);
                MMQ2_SCALE32(7, 1)
                __builtin_amdgcn_sched_barrier(0);
#undef MMQ2_ISSUE32
#undef MMQ2_SCALE32
            }
        };
        tile(std::integral_constant<int, 0>{});                   // written out: as a loop over tt the _1 members' bodies exceed the unroller's size limit
        if constexpr (TT > 1) tile(std::integral_constant<int, 1>{});
        if constexpr (TT > 2) tile(std::integral_constant<int, 2>{});
    }
    float accf[TT][16];
#pragma unroll
    for (int tt = 0; tt < TT; tt++)
#pragma unroll
        for (int r = 0; r < 16; r++) accf[tt][r] = acc[tt][r];
    mmq2_store<TT>(accf, a, m, r0 + l31, W.rows, t0, my_tiles, hh);
}

template <int T, int TT>
static void launch_q32_tt(dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A) {
    using S = Mmq2Stage80<TT>;
    constexpr size_t lds = 2 * (S::BYTES + (T == GT_Q4_1 || T == GT_Q5_1 ? S::DS : 0)) + 16384;   // the kernel's STAGE, twice, + the four waves' transpose scratch
    static bool attr = false;
    if (!attr) { HIP_IGNORE(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mmq2_q32<T, TT>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024)); attr = true; }
    hipLaunchKernelGGL((k_mmq2_q32<T, TT>), grid, dim3(256), lds, s, a, A);
}
template <int T>
static void launch_q32_t(dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A) {
    switch (a.tiles_per_chunk) {
    case 1: launch_q32_tt<T, 1>(grid, s, a, A); break;
    case 2: launch_q32_tt<T, 2>(grid, s, a, A); break;
    case 3: launch_q32_tt<T, 3>(grid, s, a, A); break;
    default: throw HipError{hipErrorInvalidValue, "mmq2: bad chunking", __FILE__, __LINE__};
    }
}
// VGPRs / scratch bytes per kernel (budget: <= 256 VGPRs, two workgroups per CU):        TT = 1        2        3
//                                                                         Q8_0        153 / 0   184 / 0   206 / 0
//                                                                         Q5_0        155 / 0   184 / 0   206 / 0
//                                                                         Q4_1        165 / 0   194 / 0   218 / 0
//                                                                         Q5_1        176 / 0   206 / 0   230 / 0
void launch_mmq2_q32(int type, dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A) {
    switch (type) {
    case GT_Q8_0: launch_q32_t<GT_Q8_0>(grid, s, a, A); break;
    case GT_Q5_0: launch_q32_t<GT_Q5_0>(grid, s, a, A); break;
    case GT_Q4_1: launch_q32_t<GT_Q4_1>(grid, s, a, A); break;
    case GT_Q5_1: launch_q32_t<GT_Q5_1>(grid, s, a, A); break;
    default: throw HipError{hipErrorInvalidValue, "mmq2: not a 32-weight-block member", __FILE__, __LINE__};
    }
}

}  // namespace mg4
