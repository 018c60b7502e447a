// What the kernels of the generation-2 prompt mat-mul family share (mmq2_kernels.hip: k-quants and Q4_0; mmq2_iq4.hip: IQ4_NL / IQ4_XS; mmq2_q32.hip: Q8_0 / Q5_0 / Q5_1 / Q4_1; mmq2_q2k.hip: Q2_K; mmq2_q3k.hip: Q3_K): the launch arguments, the LDS
// image of an activation stage and its LDS-DMA requests (Q8_K rows: Mmq2Stage; Q8_0 rows: Mmq2Stage80), and the result store.
#pragma once
#include "kernels.hpp"
#include "devutil.hpp"

namespace mg4 {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

namespace {
__device__ __forceinline__ float h2f_b(unsigned short h) { return __half2float(__ushort_as_half(h)); }
__device__ __forceinline__ v4i ldg16(const void *p) { return *reinterpret_cast<const v4i *>(p); }
__device__ __forceinline__ v16i zero16() { v16i z; for (int i = 0; i < 16; i++) z[i] = 0; return z; }
__device__ __forceinline__ int tok_of(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }   // MFMA 32x32 C layout: row (= token) of accumulator register `reg`
__device__ __forceinline__ long pack64(int lo, int hi) { return (long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo); }
__device__ __forceinline__ int sext6(int x) { const int yv = x ^ 0x20202020; const int s = yv & 0x20202020; return yv | (s << 1) | (s << 2); }   // 4 x (6-bit q - 32) as int8

typedef __attribute__((address_space(3))) void *lds_ptr_t;
typedef const __attribute__((address_space(1))) void *glb_ptr_t;
__device__ __forceinline__ void dma16(const void *src, unsigned char *lds_wave_base) {   // LDS[lds_wave_base + lane * 16 .. +16) <- src (per lane)
    __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)lds_wave_base, 16, 0, 0);
}
__device__ __forceinline__ void dma4(const void *src, unsigned char *lds_wave_base) {    // LDS[lds_wave_base + lane * 4 .. +4) <- src
    __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)lds_wave_base, 4, 0, 0);
}
}  // namespace

// LDS image of one activation stage (TT token tiles of one super-block):
//   q8 [TT * 32 tokens][16 chunks of 16 B], chunk c of token t stored at slot c ^ (t & 15)
//   bs [TTP * 32][16 B]  digit-split per-32 sums (TTP = TT rounded up to 2: one DMA instruction covers 64 tokens)
//   dk [TTP * 32] fp32   activation super-block scale
template <int TT> struct Mmq2Stage {
    static constexpr int TTP = (TT + 1) & ~1;
    static constexpr int Q8 = TT * 32 * 256, BS = TTP * 32 * 16, DK = TTP * 32 * 4;
    static constexpr int BYTES = Q8 + BS + DK;
};

struct Mmq2Args {
    QWeight w[3];                 // 1..3 matrices of one type and one shape; row group g belongs to matrix g / groups_each
    float *y[3];                  // outputs, [N][ldy] each (K split: slab z at y + z * slab_stride)
    const float *res[3];          // optional residual inputs (only without a K split)
    int n_mat, groups_each;       // row groups (of 128 rows) per matrix
    int N, ldy;
    int n_tiles, tiles_per_chunk; // token tiles of 32 in total / per grid.y chunk
    int sb_per_split;             // super-blocks per grid.z slice
    long long slab_stride;        // floats between K-split slabs
};

// Requests stage `sb` of this chunk into LDS buffer `st` (all WPB waves of the workgroup take part; every request is unconditional, indices clamped).  n_q8: q8 wave-instructions
// (4 tokens each) that carry live tokens -- the single-wave form (batched decode: a few rows) skips the rest; their LDS rows keep stale bytes that only ever reach
// accumulator registers of tokens >= N, which are never stored.
template <int TT, int WPB>
__device__ __forceinline__ void mmq2_stage_load(const ActQ &A, int K, int NSB, int N, int t0, int sb, unsigned char *st, int wv, int lane, int n_q8) {
    using S = Mmq2Stage<TT>;
    // q8: TT * 8 wave-instructions of 4 tokens x 16 chunks; wave wv issues instructions wv * (8 TT / WPB) .. + 8 TT / WPB - 1
#pragma unroll
    for (int k = 0; k < 8 * TT / WPB; k++) {
        const int ii = wv * (8 * TT / WPB) + k;
        const int tl = 4 * ii + (lane >> 4);                 // token within the chunk
        const int c = (lane & 15) ^ (tl & 15);               // logical chunk that lands in slot (lane & 15)
        const int tok = min(t0 + tl, N - 1);
        if (WPB == 4 || ii < n_q8) dma16(A.q8k + (size_t)tok * K + (size_t)sb * 256 + c * 16, st + ii * 1024);
    }
    if (WPB == 1 || wv == 0) {
#pragma unroll
        for (int j = 0; j < S::TTP / 2; j++) { const int tok = min(t0 + 64 * j + lane, N - 1); dma16(A.bsq + ((size_t)tok * NSB + sb) * 16, st + S::Q8 + j * 1024); }
    }
    if (WPB == 1 || wv == 1) {
#pragma unroll
        for (int j = 0; j < S::TTP / 2; j++) { const int tok = min(t0 + 64 * j + lane, N - 1); dma4(A.dk + (size_t)tok * NSB + sb, st + S::Q8 + S::BS + j * 256); }
    }
}

// Result store: lane = weight row, accumulator register = token -> 32 consecutive floats per (register, lane half).  The residual values of a token tile are
// requested together (clamped addresses, no branch around a load) before any of them is used.
template <int TT>
__device__ __forceinline__ void mmq2_store(const float (&acc)[TT][16], const Mmq2Args &a, int m, int orow, int rows, int t0, int my_tiles, int hh) {
    float *y = a.y[m] + (size_t)blockIdx.z * a.slab_stride;
    const bool has_res = gridDim.z == 1 && a.res[m] != nullptr;
    const float *rb = has_res ? a.res[m] : y;
    const int rowc = min(orow, rows - 1);
#pragma unroll
    for (int tt = 0; tt < TT; tt++) {
        if (tt < my_tiles) {
            float rv[16];
#pragma unroll
            for (int r = 0; r < 16; r++) rv[r] = rb[(size_t)min(t0 + tt * 32 + tok_of(r, hh), a.N - 1) * a.ldy + rowc];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int tok = t0 + tt * 32 + tok_of(r, hh);
                if (tok < a.N && orow < rows) y[(size_t)tok * a.ldy + orow] = has_res ? acc[tt][r] + rv[r] : acc[tt][r];
            }
        }
    }
}

template <int TT> struct Mmq2Stage80 {
    static constexpr int TTP = (TT + 1) & ~1;
    static constexpr int Q8 = TT * 32 * 256, DS = 8 * TTP * 32 * 4;      // q8 as Mmq2Stage; scales [8 blocks][TTP * 32 tokens] fp32 (token-contiguous: 4 accumulator registers = 16 bytes)
    static constexpr int BYTES = Q8 + DS;
};
template <int TT, int WPB>
__device__ __forceinline__ void mmq2_stage_load80(const ActQ &A, int K, int N, int t0, int sb, unsigned char *st, int wv, int lane, const unsigned (&tokoff)[Mmq2Stage80<TT>::TTP / 2], int n_q8) {
    using S = Mmq2Stage80<TT>;
#pragma unroll
    for (int k = 0; k < 8 * TT / WPB; k++) {
        const int ii = wv * (8 * TT / WPB) + k;
        const int tl = 4 * ii + (lane >> 4);
        const int c = (lane & 15) ^ (tl & 15);
        const int tok = min(t0 + tl, N - 1);
        if (WPB == 4 || ii < n_q8) dma16(A.q80 + (size_t)tok * K + (size_t)sb * 256 + c * 16, st + ii * 1024);
    }
    // scales: instruction (b, j) = block b of the super-chunk, tokens 64 j + lane; wave wv takes blocks wv and wv + 4 (the single wave: all 8).  tokoff[j] (this lane's row
    // offset into d0) is computed once by the caller: rebuilding 64-bit addresses per instruction is cheaper than the 16 hoisted pointer pairs hipcc otherwise keeps (and spills)
    constexpr int HJ = S::TTP / 2;
#pragma unroll
    for (int j = 0; j < HJ; j++) {
        if (WPB == 4) {
            const float *pj = A.d0 + (size_t)tokoff[j] + (size_t)sb * 8 + wv;
            dma4(pj, st + S::Q8 + (wv * S::TTP * 32 + 64 * j) * 4);
            dma4(pj + 4, st + S::Q8 + ((wv + 4) * S::TTP * 32 + 64 * j) * 4);
        } else {
            const float *pj = A.d0 + (size_t)tokoff[j] + (size_t)sb * 8;
#pragma unroll
            for (int b = 0; b < 8; b++) dma4(pj + b, st + S::Q8 + (b * S::TTP * 32 + 64 * j) * 4);
        }
    }
}
// the IQ4 members (mmq2_iq4.hip): tiles_per_chunk 1..3, grid and arguments as launch_mmq2_set prepares them for every member
void launch_mmq2_iq4(int type, dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A);
// the Q8_0 / Q5_0 / Q5_1 / Q4_1 members (mmq2_q32.hip): likewise; Q4_1 / Q5_1 read A.d1 and A.s1 instead of A.d0
void launch_mmq2_q32(int type, dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A);
// the Q2_K member (mmq2_q2k.hip): likewise; Q8_K rows, reads A.q8k and A.dk (the staged per-32 sums go unread)
void launch_mmq2_q2k(int type, dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A);
// the Q3_K member (mmq2_q3k.hip): likewise
void launch_mmq2_q3k(int type, dim3 grid, hipStream_t s, const Mmq2Args &a, const ActQ &A);

}  // namespace mg4
