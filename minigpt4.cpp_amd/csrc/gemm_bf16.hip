// Prompt rows (N >= 16) against an unquantised BF16 matrix on the bf16 matrix cores: y[t][r] = W[r] . act[t] (+ residual[t][r]).
//
// ggml's arithmetic for the type (vec_dot_type BF16): the activation row rounded to bfloat16 (k_rms_quant / k_silu_mul_quant leave it in ActQ::xh's storage), exact
// bf16 x bf16 products, fp32 accumulation -- which is v_mfma_f32_32x32x16_bf16.  Both operands are K-contiguous (rows [N][K], weights [n_out][K]), so 16 bytes of either
// are one lane's MFMA fragment (8 values of K) as they stand: nothing is converted, transposed or repacked on the way.
//
// k_gemm_bf16<TT>
//   * Workgroup tile: 128 outputs x 32 TT tokens (TT = 1 .. 4), 256 threads = 4 waves.  Wave w owns outputs 32 w .. 32 w + 31 against all TT token tiles: TT accumulator
//     sets of 16 floats.  The weights are the MFMA's A operand (lane & 31 = output), the rows its B operand (lane & 31 = token), so a lane ends up with 4 x 4
//     CONSECUTIVE outputs of one token: the store is four 16-byte writes per token tile.
//     TT follows N as k_mmq2_*'s does: n_tiles = ceil(N / 32) is cut into ceil(n_tiles / 4) chunks of equal size (grid.y), TT = tiles per chunk (N = 142: 5 tiles ->
//     2 chunks of 3; N = 512: 4 chunks of 4), so the weights are streamed once per <= 128 rows.
//   * K step 64 = 128 bytes of every row of the tile = 8 chunks of 16 bytes.  Thread (r = tid / 8, c = tid % 8) copies chunk c of rows r, r + 32, ...: eight
//     neighbouring lanes read one whole 128-byte line, 4 + TT 16-byte global loads per thread and step, held in registers and written to LDS with ds_write_b128.
//     LDS ring of depth 2: the loads of step k + 1 are issued before the MFMAs of step k and written behind them into the other buffer; one barrier per step.
//     2 x (128 + 32 TT) x 128 bytes = 40 / 48 / 56 / 64 KiB.
//   * Swizzle instead of padding: chunk c of row r sits at chunk c ^ ((r >> 1) & 7) of its 128-byte row.  A fragment read (ds_read_b128) has lanes 0 .. 31 on 32
//     consecutive rows at ONE logical chunk: any 16 consecutive rows then cover all 16 16-byte slots of a 256-byte span of the 64 banks (r & 1 picks the half,
//     (r >> 1) & 7 the slot) -- no two lanes of a 16-lane group share a bank; the writes (8 lanes = one row's 8 chunks, 16 lanes = two rows) are a permutation of a
//     contiguous 256 bytes.  Unpadded, every row of a column would start at the same bank.
//   * Per wave and step: 4 k-substeps x (1 + TT reads of 1 KiB, TT MFMAs).
//   * Ragged edges: rows past n_out and tokens past N are clamped to the last valid one when loaded and masked when stored; the chunks of a last step past the K
//     range are replaced by zeros in the registers (K is a multiple of 8, so a chunk is inside or outside as a whole).
//   * Epilogue: optional residual (same [t][r] layout and ldy as y), ldy >= n_out; 16-byte stores where y, ldy and the 4-output group allow, scalar ones otherwise.
//
// Filling 256 CUs.  At the 13B widths a prompt of 142 rows is n_out = 5120 -> 40 row groups x 2 chunks = 80 workgroups, w1 | w3 (13824 outputs) 216: a few dozen to a
// couple of hundred tiles, and smaller tiles would only re-stream the activation rows more often.  So K is split over grid.z through the workspace that travels with the
// rows (ActQ::ws), exactly as launch_mmq2_set does it: the launcher adds slices while the grid is below one workgroup per CU, a slice keeps >= 512 of K (8 steps) and the
// slabs fit; slice z writes its partial tile to slab z and launch_slab_flush (k_mmq2_reduce_set) adds the slabs in fixed order, with the residual.  The flat combine
// walks N x ldy floats, so K is split only where ldy == n_out and that count is a multiple of 4.  wq .. w2 are one launch per matrix.
//
// Registers and LDS (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): the table at launch_gemm_bf16; no instance uses scratch memory.
#include "kernels.hpp"

#include <algorithm>

namespace mg4 {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

struct GemmBf16Args {
    const uint8_t *W, *X;        // [n_out][K], [N][K] bfloat16
    float *y; const float *res;  // [N][ldy]; with a K split: slab 0 of the workspace, no residual
    long long slab_stride;       // floats between the slabs of consecutive K slices
    int N, n_out, K, ldy, tiles_per_chunk, k_per_slice, vec;   // vec: y (and res) admit 16-byte accesses
};

constexpr int GB_ROWS = 128, GB_KSTEP = 64, GB_CHUNKS = GB_KSTEP / 8;
__device__ __forceinline__ int gb_slot(int row, int c) { return row * GB_CHUNKS + (c ^ ((row >> 1) & 7)); }

template <int TT>
__global__ __launch_bounds__(256) void k_gemm_bf16(const GemmBf16Args a) {
    extern __shared__ __attribute__((aligned(16))) int4 smem_gb[];   // [2][128 weight rows + 32 TT token rows][8 chunks]
    constexpr int STAGE = (GB_ROWS + 32 * TT) * GB_CHUNKS;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = tid >> 3, lc = tid & 7;
    const int row0 = blockIdx.x * GB_ROWS, t0 = blockIdx.y * a.tiles_per_chunk * 32;
    const int K = a.K, kb = blockIdx.z * a.k_per_slice, ke = min(K, kb + a.k_per_slice);
    // this thread's rows of the tile: clamped, so that every load has a valid address
    const uint8_t *wp[4], *xp[TT];
#pragma unroll
    for (int j = 0; j < 4; j++) wp[j] = a.W + (size_t)min(row0 + lr + 32 * j, a.n_out - 1) * K * 2;
#pragma unroll
    for (int j = 0; j < TT; j++) xp[j] = a.X + (size_t)min(t0 + lr + 32 * j, a.N - 1) * K * 2;
    int4 wreg[4], xreg[TT];
    auto gload = [&](int k0) {
        const int k = k0 + lc * 8;
        const bool in = k < ke;
        const size_t off = (size_t)(in ? k : kb) * 2;
        const int keep = in ? -1 : 0;              // (a select between two int4 values goes through scratch memory)
#pragma unroll
        for (int j = 0; j < 4; j++) { const int4 v = *reinterpret_cast<const int4 *>(wp[j] + off); wreg[j] = make_int4(v.x & keep, v.y & keep, v.z & keep, v.w & keep); }
#pragma unroll
        for (int j = 0; j < TT; j++) { const int4 v = *reinterpret_cast<const int4 *>(xp[j] + off); xreg[j] = make_int4(v.x & keep, v.y & keep, v.z & keep, v.w & keep); }
    };
    auto lstore = [&](int buf) {
        int4 *st = smem_gb + buf * STAGE;
#pragma unroll
        for (int j = 0; j < 4; j++) st[gb_slot(lr + 32 * j, lc)] = wreg[j];
#pragma unroll
        for (int j = 0; j < TT; j++) st[GB_ROWS * GB_CHUNKS + gb_slot(lr + 32 * j, lc)] = xreg[j];
    };
    f32x16_t acc[TT];
#pragma unroll
    for (int j = 0; j < TT; j++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[j][i] = 0.0f;
    gload(kb);
    lstore(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = kb; k0 < ke; k0 += GB_KSTEP) {
        const bool more = k0 + GB_KSTEP < ke;      // workgroup-uniform
        if (more) gload(k0 + GB_KSTEP);
        const int4 *st = smem_gb + buf * STAGE;
#pragma unroll
        for (int kk = 0; kk < GB_KSTEP / 16; kk++) {   // the MFMA's K layout: lane half hh holds k = 8 hh .. 8 hh + 7 of the 16
            const bf16x8_t wf = __builtin_bit_cast(bf16x8_t, st[gb_slot(32 * wv + l31, 2 * kk + hh)]);
#pragma unroll
            for (int j = 0; j < TT; j++) {
                const bf16x8_t xf = __builtin_bit_cast(bf16x8_t, st[GB_ROWS * GB_CHUNKS + gb_slot(32 * j + l31, 2 * kk + hh)]);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, acc[j], 0, 0, 0);
            }
        }
        if (more) lstore(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    // accumulator i of a lane: output 8 (i / 4) + 4 hh + i % 4 of the wave's 32, token l31 of the tile
    float *y = a.y + (size_t)blockIdx.z * a.slab_stride;
#pragma unroll
    for (int j = 0; j < TT; j++) {
        const int t = t0 + 32 * j + l31;
        if (t >= a.N) continue;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int r = row0 + 32 * wv + 8 * g + 4 * hh;
            const size_t o = (size_t)t * a.ldy + r;
            if (a.vec && r + 3 < a.n_out) {
                float4 v = make_float4(acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]);
                if (a.res) { const float4 q = *reinterpret_cast<const float4 *>(a.res + o); v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
                *reinterpret_cast<float4 *>(y + o) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) if (r + e < a.n_out) y[o + e] = a.res ? acc[j][4 * g + e] + a.res[o + e] : acc[j][4 * g + e];
            }
        }
    }
}

template <int TT>
static void launch_gemm_bf16_tt(dim3 grid, hipStream_t s, const GemmBf16Args &a) {
    constexpr size_t lds = (size_t)2 * (GB_ROWS + 32 * TT) * GB_CHUNKS * 16;
    static bool attr = false;
    if (!attr) { HIP_IGNORE(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gemm_bf16<TT>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024)); attr = true; }
    hipLaunchKernelGGL((k_gemm_bf16<TT>), grid, dim3(256), lds, s, a);
}
// VGPRs + AGPRs / scratch bytes / LDS bytes / waves per SIMD by registers:   TT = 1: 50 + 16 / 0 / 40960 / 7     2: 70 + 32 / 0 / 49152 / 4
//                                                                             3: 68 + 48 / 0 / 57344 / 4     4: 77 + 64 / 0 / 65536 / 3
bool launch_gemm_bf16(const QWeight &W, const ActQ &A, int N, float *y, int ldy, const float *residual, const LaunchTuning &tune, hipStream_t s) {
    if (W.type != GT_BF16 || N < 1 || W.cols % 8 || !A.xh || ldy < W.rows) return false;
    GemmBf16Args a{};
    a.W = W.qs; a.X = reinterpret_cast<const uint8_t *>(A.xh); a.y = y; a.res = residual;
    a.N = N; a.n_out = W.rows; a.K = W.cols; a.ldy = ldy;
    const int n_tiles = (N + 31) / 32, n_chunks = (n_tiles + 3) / 4;
    a.tiles_per_chunk = (n_tiles + n_chunks - 1) / n_chunks;
    const int groups = (W.rows + GB_ROWS - 1) / GB_ROWS, wgs = groups * n_chunks, steps = (W.cols + GB_KSTEP - 1) / GB_KSTEP;
    const size_t out_floats = (size_t)N * ldy;
    // K split: slices while the grid is below one workgroup per CU, >= 8 steps (512 of K) per slice, the slabs fit the workspace, and the flat combine applies
    const bool can_split = A.ws && ldy == W.rows && out_floats % 4 == 0 && ((uintptr_t)y & 15) == 0 && (!residual || ((uintptr_t)residual & 15) == 0);
    int ks = 1;
    if (can_split) {
        while (wgs * ks < tune.cus && steps / (ks + 1) >= 8 && (size_t)(ks + 1) * out_floats <= A.ws_floats) ks++;
        if (tune.mmq_ks > 0) ks = std::max(1, std::min(tune.mmq_ks, std::min(steps, (int)std::min<size_t>(64, A.ws_floats / out_floats))));
    }
    const int steps_per_slice = (steps + ks - 1) / ks;
    ks = (steps + steps_per_slice - 1) / steps_per_slice;
    a.k_per_slice = steps_per_slice * GB_KSTEP;
    if (ks > 1) { a.y = A.ws; a.res = nullptr; a.slab_stride = (long long)out_floats; }
    a.vec = ldy % 4 == 0 && ((uintptr_t)a.y & 15) == 0 && (!a.res || ((uintptr_t)a.res & 15) == 0);
    const dim3 grid((unsigned)groups, (unsigned)n_chunks, (unsigned)ks);
    switch (a.tiles_per_chunk) {
    case 1: launch_gemm_bf16_tt<1>(grid, s, a); break;
    case 2: launch_gemm_bf16_tt<2>(grid, s, a); break;
    case 3: launch_gemm_bf16_tt<3>(grid, s, a); break;
    default: launch_gemm_bf16_tt<4>(grid, s, a); break;
    }
    if (ks > 1) {
        SlabSrc src; src.ws = A.ws; src.ks = ks; src.stride = (long long)out_floats; src.n = 1;
        src.y[0] = y; src.res[0] = residual; src.mbase[0] = A.ws; src.mks[0] = ks;
        launch_slab_flush(src, s);
    }
    return true;
}

}  // namespace mg4
