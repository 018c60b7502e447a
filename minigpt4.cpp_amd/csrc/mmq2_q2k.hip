// Q2_K member of the generation-2 prompt mat-mul family (mmq2_kernels.hip has the structure's description and the other k-quant members; the launch arguments, the
// activation staging and the result store are the family's own: mmq2_common.hpp).  Until this kernel, N >= 5 rows against a Q2_K matrix ran on k_mul_mat<T, 2, 4>: v_dot4 on
// the vector ALU and one pass over the weights per FOUR rows.
//
// k_mmq2_q2k<TT> keeps the family's skeleton (4 waves x 32 weight rows x TT <= 3 token tiles x one K range; Q8_K activation rows by LDS-DMA, source-side swizzled, double
// buffered: Mmq2Stage and mmq2_stage_load as they are; one barrier per super-block; lane = weight row) and puts the SUB-BLOCK SCALES INSIDE THE int8 OPERANDS, which no
// other k-quant admits without a digit split (mmq2_kernels.hip's header: measured and removed three times): a Q2_K sub-block scale has 4 bits and a quant 2, so
// sc_j * q <= 15 * 3 = 45 is ONE int8 byte.
//   * Main term.  Lane half hh of row l31 owns sub-block 2 b + hh of unit b (the MFMA's K layout: half hh holds k = 16 hh .. 16 hh + 15), i.e. the repacked word P_hh of
//     the unit.  Its B operand is four dwords of sc_j * q, each built by ONE v_perm_b32: selector = the 2-bit quant dword (P >> 2 k) & 0x03030303, table =
//     {0, sc, 2 sc, 3 sc} = sc * 0x03020100 in one register (one v_mul_lo_u32 per sub-block and lane).  11 vector operations per unit and lane (3 shifts, 4 ands,
//     4 perms), paid once per super-block and row tile and reused by every token tile.  The other full-rate form, v_pk_mul_lo_u16 by the scale, needs the four quants of a
//     dword spread over two registers of 16-bit lanes and merged again (two ands, a shift, two multiplies, a shift-or per dword: 6 against 3) -- the ISA listing of
//     either form has nothing else in the unpack, so the lookup form is the one built.
//     The eight K = 32 v_mfma_i32_32x32x32_i8 of a super-block CHAIN into one int32 accumulator set per token tile: i0 = sum_j sc_j sum q a, |i0| <= 256 * 45 * 127 < 2^21,
//     exact, and exact again as a float.  The per-(row, token, sub-block) integer multiply-adds of the other k-quant members (their bound: 84 % VALU issue) do not exist.
//   * Min term.  A second chain of eight MFMAs against the same A fragments, B operand = m_j replicated over the sub-block's 16 bytes (m * 0x01010101, one v_perm_b32
//     with selector 0): i1 = sum_j m_j bsum_j exactly (<= 256 * 15 * 127), with no staged sums -- the stage's bsq digits are per 32 activations, Q2_K's sub-blocks are 16 wide; they are staged by the
//     family's loader and go unread, as in k_mmq2_iq4<XS>.  (A cheaper exact form exists on paper -- two K = 16 MFMAs on digit-split per-16 sums -- but it needs a plane
//     the activation quantiser does not write; not built.)
//   * Per super-block and output: acc = fma(d * d_a, (float)i0, acc); acc = fma(-(dmin * d_a), (float)i1, acc) -- the products and the order of Tr<GT_Q2_K>::terms /
//     ref_chunk, so without a K split every output equals k_mul_mat_ref's value bit for bit (parity mode's prompt rows; tests/test_gpu_mmq2_q2k.py).
//     16 MFMAs (Q6_K's count) and 4 LDS reads + 32 conversions + 32 products + 32 fma's per super-block and token tile.  The MFMAs of token tile tt + 1 are issued
//     before the conversions and fma's of tile tt (two result sets); each tile's scale arithmetic stays there (the accumulator pin and sched_barrier pattern of k_mmq2_q40).
// Weights: a row's super-block is 64 (qs) + 16 (sc) + 4 (d) bytes, half of Q4_0's main plane.  Chosen: ONE super-block per stage, main plane as 16 rows x 64 contiguous
// bytes per request (two requests per lane and super-block), not a two-super-block stage of 8 rows x 128 bytes: the stage, the barrier count per super-block and
// sb_per_split stay the family's, an odd super-block count (K = 256, K = 768) needs no tail form, and the second half of every 128-byte line is the NEXT super-block's
// request (an L2 hit).  The transpose scratch shrinks to 2 KiB per wave: [32 rows][4 pieces x 16 B], piece p of row r at slot p ^ ((r >> 1) ^ (r >> 3)) & 3; a lane reads
// its row's four pieces ({P0, P1} of units 2 j, 2 j + 1) and keeps the word of its half.
// LDS per workgroup: 2 x Mmq2Stage<TT>::BYTES + 4 x 2048 = 26112 / 44544 / 62464 bytes at TT = 1 / 2 / 3 (61 KiB at most: two workgroups take 122 of the CU's 160 KiB).
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): the table at launch_mmq2_q2k; no instance uses scratch memory.
#include "mmq2_common.hpp"

namespace mg4 {

template <int TT>
__global__ __launch_bounds__(256, 2) void k_mmq2_q2k(const Mmq2Args a, const ActQ A) {
    using S = Mmq2Stage<TT>;
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem_mmq2[];   // [2 activation stages][4 waves x 2 KiB weight transpose scratch]
    const int lane = threadIdx.x & 63, hh = lane >> 5, l31 = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = blockIdx.x / a.groups_each, g = blockIdx.x - m * a.groups_each;
    const QWeight W = a.w[m];
    const int K = W.cols, U = K / 32, NSB = K / 256, N = a.N;
    const int r0 = (g * 4 + wv) * 32;
    const int row = min(r0 + l31, W.rows - 1);
    const int tile0 = blockIdx.y * a.tiles_per_chunk, my_tiles = min(TT, a.n_tiles - tile0), t0 = tile0 * 32;
    const int sb0 = blockIdx.z * a.sb_per_split, sb1 = min(NSB, sb0 + a.sb_per_split);
    unsigned char *scratch = smem_mmq2 + 2 * S::BYTES + wv * 2048;

    typedef float v16f_t __attribute__((ext_vector_type(16)));
    v16f_t acc[TT];
#pragma unroll
    for (int tt = 0; tt < TT; tt++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[tt][r] = 0.0f;

    // coalesced weight requests: main plane, instruction n: rows 16 n .. 16 n + 15 x the super-block's 64 contiguous bytes (4 lanes of 16 bytes per row); per row the
    // super-block's 16 {scale | min << 4} bytes (both lane halves request the same 16 bytes: one cache line) and its {d, dmin}
    struct Raw { v4i q[2]; v4i h; unsigned dm; };
    const unsigned char *wq[2];
#pragma unroll
    for (int n = 0; n < 2; n++) wq[n] = W.qs + ((size_t)min(r0 + 16 * n + (lane >> 2), W.rows - 1) * U * 8 + (lane & 3) * 16);
    const unsigned char *wh = W.sc + (size_t)row * U * 2, *wd = W.d + (size_t)row * NSB * 4;
    auto fetch = [&](int sb, Raw &w) {
#pragma unroll
        for (int n = 0; n < 2; n++) w.q[n] = ldg16(wq[n] + (size_t)sb * 64);
        w.h = ldg16(wh + (size_t)sb * 16);
        w.dm = *reinterpret_cast<const unsigned *>(wd + (size_t)sb * 4);
    };
    auto slot = [](int r) { return ((r >> 1) ^ (r >> 3)) & 3; };   // 16 consecutive rows x one piece: 16 different 16-byte bank groups, with 32 or 64 banks
    unsigned sw_addr[2], sr_addr[4], a_addr[8];
#pragma unroll
    for (int n = 0; n < 2; n++) { const int r = 16 * n + (lane >> 2); sw_addr[n] = (unsigned)(r * 64 + (((lane & 3) ^ slot(r)) << 4)); }
#pragma unroll
    for (int j = 0; j < 4; j++) sr_addr[j] = (unsigned)(l31 * 64 + ((j ^ slot(l31)) << 4));              // both lane halves read piece j of their row (hh selects the word)
    const int v = hh ^ (lane & 15);
#pragma unroll
    for (int b = 0; b < 8; b++) a_addr[b] = (unsigned)(l31 * 256 + (((2 * b) ^ v) << 4));                // elements 32 b + 16 hh .. + 15 of token l31
    const unsigned dk_addr = (unsigned)(S::Q8 + S::BS + 16 * hh);
    const int sh8 = 8 * hh;

    Raw raw;
    fetch(sb0, raw);
    mmq2_stage_load<TT, 4>(A, K, NSB, N, t0, sb0, smem_mmq2, wv, lane, 8 * TT);
    for (int sb = sb0; sb < sb1; sb++) {
        const int buf = (sb - sb0) & 1;
        unsigned char *st = smem_mmq2 + buf * S::BYTES;
        __syncthreads();                                           // own DMA + weight loads done, then everybody's
        // ---- this super-block's weights: transpose through LDS (same wave writes and reads: LDS operations of a wave execute in order), then quant -> sc * quant by
        // table lookup, straight into the eight B operands; the eight min operands are one register each (replicated into four where the MFMA is issued)
#pragma unroll
        for (int n = 0; n < 2; n++) *reinterpret_cast<v4i *>(scratch + sw_addr[n]) = raw.q[n];
        v4i wb[8];
        unsigned bm[8];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const v4i q = *reinterpret_cast<const v4i *>(scratch + sr_addr[j]);                          // {P0, P1} of unit 2 j | {P0, P1} of unit 2 j + 1
            const unsigned sm = (unsigned)raw.h[j] >> sh8;                                               // byte 0: {scale | min << 4} of sub-block 2 (2 j) + hh, byte 2: of 2 (2 j + 1) + hh
#pragma unroll
            for (int o = 0; o < 2; o++) {
                const int b = 2 * j + o;
                const unsigned P = (unsigned)(hh ? q[2 * o + 1] : q[2 * o]);
                const unsigned tab = ((sm >> (16 * o)) & 0xFu) * 0x03020100u;                            // bytes {0, sc, 2 sc, 3 sc}: 3 sc <= 45, no carry between bytes (a 32-bit multiply: the constant has more than 24 bits)
                bm[b] = __builtin_amdgcn_perm(0u, (sm >> (16 * o + 4)) & 0xFu, 0u);                      // m in all four bytes
#pragma unroll
                for (int k = 0; k < 4; k++) wb[b][k] = (int)__builtin_amdgcn_perm(0u, tab, (P >> (2 * k)) & 0x03030303u);   // selector bytes 0..3 pick the table's bytes
            }
        }
        const float dw = h2f_b(raw.dm & 0xFFFF), ndmin = -h2f_b(raw.dm >> 16);
        __builtin_amdgcn_sched_barrier(0);                         // the raw registers are dead from here: the next super-block's loads reuse them
        {
            const int sbn = min(sb + 1, sb1 - 1);
            fetch(sbn, raw);
            mmq2_stage_load<TT, 4>(A, K, NSB, N, t0, sbn, smem_mmq2 + (buf ^ 1) * S::BYTES, wv, lane, 8 * TT);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- token tiles: two chains of eight MFMAs per tile (main, min) on the same A fragments; tile tt + 1's chains are issued before tile tt's results are scaled
        v16i I0[2], I1[2];
#define MMQ2_ISSUE2K(tt, k) { const unsigned char *sq_ = st + (tt) * 8192;                                                                        \
                              _Pragma("unroll") for (int b = 0; b < 8; b++) {                                                                     \
                                  const v4i af_ = *reinterpret_cast<const v4i *>(sq_ + a_addr[b]);                                                \
                                  int mb_ = (int)bm[b]; asm volatile("" : "+v"(mb_));   /* replicated HERE: hoisted, the eight min operands would hold 32 registers */ \
                                  const v4i bm_ = {mb_, mb_, mb_, mb_};                                                                           \
                                  I0[k] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af_, wb[b], b ? I0[k] : zero16(), 0, 0, 0);                       \
                                  I1[k] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af_, bm_, b ? I1[k] : zero16(), 0, 0, 0); } }
#define MMQ2_SCALE2K(tt, k) { _Pragma("unroll") for (int q4 = 0; q4 < 4; q4++) {                                                                  \
                                  const v4f da = *reinterpret_cast<const v4f *>(st + dk_addr + (tt) * 128 + q4 * 32);   /* tokens 8 q4 + 4 hh + 0..3 = registers 4 q4 .. 4 q4 + 3 */ \
                                  _Pragma("unroll") for (int e = 0; e < 4; e++) { const int r = 4 * q4 + e;                                       \
                                      acc[tt][r] = fmaf(dw * da[e], (float)I0[k][r], acc[tt][r]);                                                 \
                                      acc[tt][r] = fmaf(ndmin * da[e], (float)I1[k][r], acc[tt][r]); } }                                          \
                              asm volatile("" : "+v"(acc[tt])); }   /* keeps the tile's scale arithmetic here (k_mmq2_q40) */
        if (0 < my_tiles) MMQ2_ISSUE2K(0, 0)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (TT > 1) { if (1 < my_tiles) MMQ2_ISSUE2K(1, 1) }
        if (0 < my_tiles) MMQ2_SCALE2K(0, 0)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (TT > 2) { if (2 < my_tiles) MMQ2_ISSUE2K(2, 0) }
        if constexpr (TT > 1) { if (1 < my_tiles) MMQ2_SCALE2K(1, 1) }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (TT > 2) { if (2 < my_tiles) MMQ2_SCALE2K(2, 0) }
        __builtin_amdgcn_sched_barrier(0);
#undef MMQ2_ISSUE2K
#undef MMQ2_SCALE2K
    }
    float accf[TT][16];
#pragma unroll
    for (int tt = 0; tt < TT; tt++)
#pragma unroll
        for (int r = 0; r < 16; r++) accf[tt][r] = acc[tt][r];
    mmq2_store<TT>(accf, a, m, r0 + l31, W.rows, t0, my_tiles, hh);
}

template <int TT>
static void launch_q2k_tt(dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A) {
    constexpr size_t lds = 2 * Mmq2Stage<TT>::BYTES + 4 * 2048;   // the two stages + the four waves' transpose scratch
    static bool attr = false;
    if (!attr) { HIP_IGNORE(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mmq2_q2k<TT>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024)); attr = true; }
    hipLaunchKernelGGL((k_mmq2_q2k<TT>), grid, dim3(256), lds, s, a, A);
}
// VGPRs / scratch bytes per kernel (budget: <= 256 VGPRs, two workgroups per CU):        TT = 1        2        3
//                                                                         Q2_K        146 / 0   216 / 0   242 / 0
void launch_mmq2_q2k(int type, dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A) {
    if (type != GT_Q2_K) throw HipError{hipErrorInvalidValue, "mmq2: not the Q2_K member", __FILE__, __LINE__};
    switch (a.tiles_per_chunk) {
    case 1: launch_q2k_tt<1>(grid, s, a, A); break;
    case 2: launch_q2k_tt<2>(grid, s, a, A); break;
    case 3: launch_q2k_tt<3>(grid, s, a, A); break;
    default: throw HipError{hipErrorInvalidValue, "mmq2: bad chunking", __FILE__, __LINE__};
    }
}

}  // namespace mg4
