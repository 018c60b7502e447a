// Q3_K member of the generation-2 prompt mat-mul family (mmq2_kernels.hip has the structure's description and the other k-quant members; the launch arguments, the
// activation staging and the result store are the family's own: mmq2_common.hpp).  Until this kernel a Q3_K matrix was held as a value-identical Q6_K image and N >= 5
// rows ran on k_mmq2_q6k: 16 MFMAs per super-block and token tile plus the per-(row, token, sub-block) integer multiply-adds by the sub-block scales.
//
// k_mmq2_q3k<TT> keeps k_mmq2_q2k's skeleton (4 waves x 32 weight rows x TT <= 3 token tiles x one K range; Q8_K activation rows by LDS-DMA, double buffered; one barrier
// per super-block; lane = weight row; the 2-bit plane requested as 16 rows x 64 bytes and transposed through 2 KiB of LDS per wave) and, like it, puts the SUB-BLOCK SCALES
// INSIDE THE int8 OPERANDS -- with the sign turned round.  A Q3_K sub-block scale is sc = s6 - 32 in [-32, 31] and a weight q = code - 4 in [-4, 3]: sc * q lies in
// [-124, 128] and misses int8 by ONE value (sc = -32, q = -4: an all-zero block), the NEGATED product -sc * q lies in [-128, 124] and is exactly one int8 byte.  No digit
// split, no min term, no staged sums:
//   * Operand.  Lane half hh of row l31 owns sub-block 2 b + hh of unit b (the MFMA's K layout: half hh holds k = 16 hh .. 16 hh + 15).  Its B operand is four dwords of
//     -sc * (code - 4), each built by ONE v_perm_b32(T1, T0, codes): codes = (P >> 2 k) & 0x03030303 | hmask bit at bit 2 (one shift and one v_and_or of the transposed
//     high-bit word), {T0, T1} = the eight possible bytes {4 sc, 3 sc, 2 sc, sc | 0, -sc, -2 sc, -3 sc} mod 256.  The table of a scale is READ, not computed: 64 entries
//     x 8 bytes in LDS, written once per workgroup, indexed by the scale (one v_bfe_i32, one ds_read_b64 per sub-block and lane; per-byte arithmetic on a signed scale
//     costs two packed multiplies and a byte merge per table dword).  22 vector operations per unit and lane against Q2_K's 11, paid once per super-block and row tile.
//   * The eight K = 32 v_mfma_i32_32x32x32_i8 of a super-block CHAIN into one int32 accumulator set per token tile: i = -sum_j sc_j sum q a, |i| <= 256 * 128 * 128 =
//     2^22, exact, and exact again as a float.  Per super-block and output: acc = fma(d * d_a, -(float)i, acc) -- the product and the order of Tr<GT_Q3_K>::terms /
//     ref_chunk, so without a K split every output equals k_mul_mat_ref's value bit for bit (parity mode's prompt rows; tests/test_gpu_q3k_native.py).
//     8 MFMAs and 1 LDS read + 16 conversions + 16 products + 16 fma's per super-block and token tile; the MFMAs of token tile tt + 1 are issued before the scaling of
//     tile tt (two result sets, the accumulator pin and sched_barrier pattern of k_mmq2_q40).
// Weights per row and super-block: 64 (low bits) + 32 (high bits) + 16 (scales) + 2 (d) bytes.  The low-bit plane goes through the transpose scratch exactly as in
// k_mmq2_q2k; the 32 high-bit bytes and the 16 scale bytes are requested per lane (its own row: both lane halves ask for the same bytes, the next three super-blocks'
// requests hit the same 128-byte line).
// LDS per workgroup: 2 x Mmq2Stage<TT>::BYTES + 4 x 2048 + 512 = 27648 / 44032 / 62976 bytes at TT = 1 / 2 / 3 (two workgroups take 123 of the CU's 160 KiB).
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): the table at launch_mmq2_q3k; no instance uses scratch memory.
#include "mmq2_common.hpp"

namespace mg4 {

template <int TT>
__global__ __launch_bounds__(256, 2) void k_mmq2_q3k(const Mmq2Args a, const ActQ A) {
    using S = Mmq2Stage<TT>;
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem_mmq2[];   // [2 activation stages][4 waves x 2 KiB weight transpose scratch][64 x 8 B operand tables]
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
    const unsigned char *tabs = smem_mmq2 + 2 * S::BYTES + 4 * 2048 + 256;       // entry of scale sc (-32 .. 31) at tabs + 8 sc
    if (threadIdx.x < 64) {   // byte c of T0 = -sc * (c - 4), byte c of T1 = -sc * c; read after the loop's first barrier
        const int sc = (int)threadIdx.x - 32;
        unsigned t0w = 0, t1w = 0;
#pragma unroll
        for (int c = 0; c < 4; c++) { t0w |= (unsigned)((4 - c) * sc & 0xFF) << (8 * c); t1w |= (unsigned)(-c * sc & 0xFF) << (8 * c); }
        *reinterpret_cast<uint2 *>(smem_mmq2 + 2 * S::BYTES + 4 * 2048 + 8 * threadIdx.x) = make_uint2(t0w, t1w);
    }

    typedef float v16f_t __attribute__((ext_vector_type(16)));
    v16f_t acc[TT];
#pragma unroll
    for (int tt = 0; tt < TT; tt++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[tt][r] = 0.0f;

    // coalesced weight requests: low-bit plane, instruction n: rows 16 n .. 16 n + 15 x the super-block's 64 contiguous bytes (4 lanes of 16 bytes per row); per row the
    // super-block's 32 high-bit bytes, its 16 int8 scales and its d
    struct Raw { v4i q[2]; v4i p[2]; v4i h; unsigned short d; };
    const unsigned char *wq[2];
#pragma unroll
    for (int n = 0; n < 2; n++) wq[n] = W.qs + ((size_t)min(r0 + 16 * n + (lane >> 2), W.rows - 1) * U * 8 + (lane & 3) * 16);
    const unsigned char *wp = W.qh + (size_t)row * U * 4, *wh = W.sc + (size_t)row * U * 2, *wd = W.d + (size_t)row * NSB * 2;
    auto fetch = [&](int sb, Raw &w) {
#pragma unroll
        for (int n = 0; n < 2; n++) w.q[n] = ldg16(wq[n] + (size_t)sb * 64);
#pragma unroll
        for (int n = 0; n < 2; n++) w.p[n] = ldg16(wp + (size_t)sb * 32 + 16 * n);
        w.h = ldg16(wh + (size_t)sb * 16);
        w.d = *reinterpret_cast<const unsigned short *>(wd + (size_t)sb * 2);
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
    const int sh8 = 8 * hh, sh4 = 4 * hh;

    Raw raw;
    fetch(sb0, raw);
    mmq2_stage_load<TT, 4>(A, K, NSB, N, t0, sb0, smem_mmq2, wv, lane, 8 * TT);
    for (int sb = sb0; sb < sb1; sb++) {
        const int buf = (sb - sb0) & 1;
        unsigned char *st = smem_mmq2 + buf * S::BYTES;
        __syncthreads();                                           // own DMA + weight loads done, then everybody's (and, the first time, the operand tables)
        // ---- this super-block's weights: low bits transposed through LDS (same wave writes and reads: LDS operations of a wave execute in order), then code ->
        // -sc * (code - 4) by table lookup, straight into the eight B operands
#pragma unroll
        for (int n = 0; n < 2; n++) *reinterpret_cast<v4i *>(scratch + sw_addr[n]) = raw.q[n];
        v4i wb[8];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const v4i q = *reinterpret_cast<const v4i *>(scratch + sr_addr[j]);                          // {P0, P1} of unit 2 j | {P0, P1} of unit 2 j + 1
            const int sm = raw.h[j] >> sh8;                                                              // byte 0: scale of sub-block 2 (2 j) + hh, byte 2: of 2 (2 j + 1) + hh
#pragma unroll
            for (int o = 0; o < 2; o++) {
                const int b = 2 * j + o;
                const unsigned P = (unsigned)(hh ? q[2 * o + 1] : q[2 * o]);
                const unsigned Hb = (unsigned)raw.p[b >> 2][b & 3] >> sh4;                               // this half's high bits: dword k at bit 8 i + k
                const int sc = (sm << (24 - 16 * o)) >> 24;                                              // v_bfe_i32
                const uint2 T = *reinterpret_cast<const uint2 *>(tabs + 8 * sc);
                wb[b][0] = (int)__builtin_amdgcn_perm(T.y, T.x, (P & 0x03030303u) | ((Hb << 2) & 0x04040404u));   // selector bytes 0..3 pick T0's bytes, 4..7 T1's
                wb[b][1] = (int)__builtin_amdgcn_perm(T.y, T.x, ((P >> 2) & 0x03030303u) | ((Hb << 1) & 0x04040404u));
                wb[b][2] = (int)__builtin_amdgcn_perm(T.y, T.x, ((P >> 4) & 0x03030303u) | (Hb & 0x04040404u));
                wb[b][3] = (int)__builtin_amdgcn_perm(T.y, T.x, ((P >> 6) & 0x03030303u) | ((Hb >> 1) & 0x04040404u));
            }
        }
        const float dw = h2f_b(raw.d);
        __builtin_amdgcn_sched_barrier(0);                         // the raw registers are dead from here: the next super-block's loads reuse them
        {
            const int sbn = min(sb + 1, sb1 - 1);
            fetch(sbn, raw);
            mmq2_stage_load<TT, 4>(A, K, NSB, N, t0, sbn, smem_mmq2 + (buf ^ 1) * S::BYTES, wv, lane, 8 * TT);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- token tiles: one chain of eight MFMAs per tile; tile tt + 1's chain is issued before tile tt's results are scaled
        v16i I0[2];
#define MMQ2_ISSUE3K(tt, k) { const unsigned char *sq_ = st + (tt) * 8192;                                                                        \
                              _Pragma("unroll") for (int b = 0; b < 8; b++) {                                                                     \
                                  const v4i af_ = *reinterpret_cast<const v4i *>(sq_ + a_addr[b]);                                                \
                                  I0[k] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af_, wb[b], b ? I0[k] : zero16(), 0, 0, 0); } }
#define MMQ2_SCALE3K(tt, k) { _Pragma("unroll") for (int q4 = 0; q4 < 4; q4++) {                                                                  \
                                  const v4f da = *reinterpret_cast<const v4f *>(st + dk_addr + (tt) * 128 + q4 * 32);   /* tokens 8 q4 + 4 hh + 0..3 = registers 4 q4 .. 4 q4 + 3 */ \
                                  _Pragma("unroll") for (int e = 0; e < 4; e++) { const int r = 4 * q4 + e;                                       \
                                      acc[tt][r] = fmaf(dw * da[e], -(float)I0[k][r], acc[tt][r]); } }                                            \
                              asm volatile("" : "+v"(acc[tt])); }   /* keeps the tile's scale arithmetic here (k_mmq2_q40) */
        if (0 < my_tiles) MMQ2_ISSUE3K(0, 0)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (TT > 1) { if (1 < my_tiles) MMQ2_ISSUE3K(1, 1) }
        if (0 < my_tiles) MMQ2_SCALE3K(0, 0)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (TT > 2) { if (2 < my_tiles) MMQ2_ISSUE3K(2, 0) }
        if constexpr (TT > 1) { if (1 < my_tiles) MMQ2_SCALE3K(1, 1) }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (TT > 2) { if (2 < my_tiles) MMQ2_SCALE3K(2, 0) }
        __builtin_amdgcn_sched_barrier(0);
#undef MMQ2_ISSUE3K
#undef MMQ2_SCALE3K
    }
    float accf[TT][16];
#pragma unroll
    for (int tt = 0; tt < TT; tt++)
#pragma unroll
        for (int r = 0; r < 16; r++) accf[tt][r] = acc[tt][r];
    mmq2_store<TT>(accf, a, m, r0 + l31, W.rows, t0, my_tiles, hh);
}

template <int TT>
static void launch_q3k_tt(dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A) {
    constexpr size_t lds = 2 * Mmq2Stage<TT>::BYTES + 4 * 2048 + 512;   // the two stages + the four waves' transpose scratch + the operand tables
    static bool attr = false;
    if (!attr) { HIP_IGNORE(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mmq2_q3k<TT>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024)); attr = true; }
    hipLaunchKernelGGL((k_mmq2_q3k<TT>), grid, dim3(256), lds, s, a, A);
}
// VGPRs / scratch bytes per kernel (budget: <= 256 VGPRs, two workgroups per CU):        TT = 1        2        3
//                                                                         Q3_K        140 / 0   180 / 0   208 / 0
void launch_mmq2_q3k(int type, dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A) {
    if (type != GT_Q3_K) throw HipError{hipErrorInvalidValue, "mmq2: not the Q3_K member", __FILE__, __LINE__};
    switch (a.tiles_per_chunk) {
    case 1: launch_q3k_tt<1>(grid, s, a, A); break;
    case 2: launch_q3k_tt<2>(grid, s, a, A); break;
    case 3: launch_q3k_tt<3>(grid, s, a, A); break;
    default: throw HipError{hipErrorInvalidValue, "mmq2: bad chunking", __FILE__, __LINE__};
    }
}

}  // namespace mg4
