// Streaming prompt attention on the fp16 matrix cores: k_attn_prefill_s<HD>.  The forms of llm_kernels.hip (k_attn_prefill_h8, k_attn_prefill_h, k_attn_prefill) keep
// the score rows of the whole context in LDS and refuse a chunk whose last key lies past 1984 keys (head size 128; 2240 at 64, 2368 at 32).  This kernel keeps NO score
// in LDS: its LDS image is one K tile and one transposed V tile of AP_KT = 64 keys (34 KiB at head size 128), whatever the context length, and the softmax state of a
// query -- running maximum, sum of exponentials -- lives in registers.
//
// Operand contract of the family: q rounded to fp16, the fp16 K / V cache rows, fp32 accumulation on v_mfma_f32_16x16x32_f16, the exponentials exp_h(tb.exp, s - max)
// (fp16 values).  The place of the normalisation differs: the LDS-row forms multiply V by p = fp16(e / sum), this one multiplies V by e and scales the fp32 result by
// 1 / sum once (tests/test_gpu_attn_stream.py has the bound's argument).
//
// Work split.  Grid (head, tile of 64 queries), the longest tile first; 4 waves, wave w owns the queries 16 w .. 16 w + 15 of the tile in both sweeps.  Key tiles past
// the tile's last query are never staged, a wave skips the tiles wholly past ITS last query, the tiles on the diagonal are masked per element.
//   sweep 1 (K only): S^T = K q^T -- the K tile is the A operand, the wave's 16 queries the B operand -- so lane (l15, l4) holds, per block of 16 keys, the scores of
//           QUERY l15 against the keys 4 l4 .. 4 l4 + 3: a query's row is spread over the 4 lanes l15, l15 + 16, .. only.  Each lane keeps the maximum of what it sees;
//           two cross-lane steps at the end of the sweep give the row's.
//   sweep 2 (K and V): the same MFMA chain on the same operands gives the same bits, so s - max is exactly 0 at the maximum and never positive.  e = exp_h(s - max)
//           goes into the lane's double sum and -- 8 values of two 16-key blocks -- IS the B operand of O^T = V^T P^T for 32 keys: the MFMA's k index is only summed
//           over, so the keys may come in the order the score fragments hold them (k = (l4, e) <-> key 16 (e >> 2) + 4 l4 + (e & 3)) as long as the A operand, V^T,
//           uses the same one.  No probability ever leaves the registers.  O^T fragments hold 4 consecutive dims of query l15: the sum the lane needs is its own, and
//           a row is stored as 16-byte pieces.
// LDS.  Kt [64][HD] fp16, the 16-byte chunk c of key j at slot c ^ (j & (HD / 8 - 1)) (the fragment reads of 16 keys x 4 chunks then touch every bank once).
// Vt [HD][APS_W] dwords, a dword = the keys (2 i, 2 i + 1) of one dim: the staging threads of a key pair first exchange halves of their 16 bytes (one takes dims 0 .. 3
// of both keys, the other 4 .. 7), so the transposition costs 4 dword writes per 16 bytes instead of 8 two-byte ones.  APS_W = 36 words per row (the 16 dims of a
// fragment read are 4 mod 8 words apart: the 8-byte reads of half a wave touch every bank once).  V is staged with 4 lanes per key (64 contiguous bytes) and 16 keys per
// wave, so the dword writes of a wave go to 8 key pairs x 4 dims.
// Both tiles are staged through registers one tile ahead (the loads of tile kt + 1 are in flight while tile kt is multiplied): two barriers per tile, as the 4-wave form.
// This file is compiled without packed fp32 instructions (csrc/Makefile).
#include "activations.hpp"
#include "kernels.hpp"

namespace mg4 {

typedef float aps4_t __attribute__((ext_vector_type(4)));
typedef _Float16 aps8_t __attribute__((ext_vector_type(8)));
constexpr int APS_KT = 64;                                        // keys per tile (= AP_KT of llm_kernels.hip)
constexpr int APS_QT = 64;                                        // queries per workgroup
constexpr int APS_W = 36;                                         // dwords per row of the transposed V tile [dim][key pair]

template <int HD>
__global__ __launch_bounds__(256) void k_attn_prefill_s(const float *__restrict__ q, const __half *__restrict__ kc, const __half *__restrict__ vc, int E, int N, const int *__restrict__ n_past,
                                                        const Tables tb, float *__restrict__ out) {
    constexpr int C8 = HD / 8, KSQ = HD / 32, DT = HD / 16, PER = APS_KT * C8 / 256, NB = APS_KT / 16;
    static_assert(PER >= 1 && PER * 4 == C8 && APS_W % 2 == 0, "V staging: 4 lanes x PER chunks per key; 8-byte fragment reads");
    __shared__ __attribute__((aligned(16))) __half Kt[APS_KT * HD];
    __shared__ __attribute__((aligned(16))) unsigned Vt[HD * APS_W];
    const int h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, l4 = lane >> 4;
    const int q0 = (int)(gridDim.y - 1 - blockIdx.y) * APS_QT, np = *n_past;
    const int T = np + min(q0 + APS_QT, N);                        // keys the last query of the tile sees
    const int nkt = (T + APS_KT - 1) / APS_KT;
    const int qrow = q0 + 16 * wave + l15, qpos = np + qrow;       // the lane's query: it sees the keys 0 .. qpos
    const int wlast = np + q0 + 16 * wave + 15;                    // the last key any query of this wave sees
    const float scale = 1.0f / sqrtf((float)HD);
    // q fragments (B operand of the scores): query l15 of the wave, dims 32 ks + 8 l4 .. + 7, rounded to fp16
    aps8_t qf[KSQ];
    {
        const float *qp = q + (size_t)min(qrow, N - 1) * E + (size_t)h * HD + 8 * l4;
#pragma unroll
        for (int ks = 0; ks < KSQ; ks++) {
            const float4 a = *reinterpret_cast<const float4 *>(qp + 32 * ks), b = *reinterpret_cast<const float4 *>(qp + 32 * ks + 4);
            const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int e = 0; e < 8; e++) qf[ks][e] = (_Float16)__half2float(f2h_rn(v[e]));
        }
    }
    // key tile `kt`, global -> registers (rows past the last key repeat it).  K: staging element e = tid + 256 u is the 16-byte chunk c of key j
    struct Stage { int4 x[PER]; };
    auto k_load = [&](int kt) {
        Stage X;
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int e = tid + 256 * u, j = e / C8, c = e - j * C8;
            X.x[u] = *reinterpret_cast<const int4 *>(kc + (size_t)min(kt * APS_KT + j, T - 1) * E + (size_t)h * HD + 8 * c);
        }
        return X;
    };
    // V: thread tid holds the chunks c = 4 u + (tid & 3) of key j = tid >> 2
    auto v_load = [&](int kt) {
        Stage X;
        const __half *vp = vc + (size_t)min(kt * APS_KT + (tid >> 2), T - 1) * E + (size_t)h * HD + 8 * (tid & 3);
#pragma unroll
        for (int u = 0; u < PER; u++) X.x[u] = *reinterpret_cast<const int4 *>(vp + 32 * u);
        return X;
    };
    auto k_write = [&](const Stage &X) {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int e = tid + 256 * u, j = e / C8, c = e - j * C8;
            *reinterpret_cast<int4 *>(Kt + j * HD + ((c ^ (j & (C8 - 1))) << 3)) = X.x[u];
        }
    };
    // the threads of keys j (even) and j + 1 are 4 lanes apart: the even one ends up with dims 8 c .. + 3 of both keys, the odd one with 8 c + 4 .. + 7
    auto v_write = [&](const Stage &X) {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int j = tid >> 2, c = 4 * u + (tid & 3);
            const bool odd = j & 1;
            const unsigned w[4] = {(unsigned)X.x[u].x, (unsigned)X.x[u].y, (unsigned)X.x[u].z, (unsigned)X.x[u].w};
            const unsigned r0 = (unsigned)__shfl_xor((int)(odd ? w[0] : w[2]), 4), r1 = (unsigned)__shfl_xor((int)(odd ? w[1] : w[3]), 4);
            const unsigned a0 = odd ? r0 : w[0], b0 = odd ? w[2] : r0, a1 = odd ? r1 : w[1], b1 = odd ? w[3] : r1;       // a: the even key's dims, b: the odd key's
            unsigned *d = Vt + (8 * c + (odd ? 4 : 0)) * APS_W + (j >> 1);
            d[0] = (a0 & 0xFFFFu) | (b0 << 16); d[APS_W] = (a0 >> 16) | (b0 & 0xFFFF0000u);
            d[2 * APS_W] = (a1 & 0xFFFFu) | (b1 << 16); d[3 * APS_W] = (a1 >> 16) | (b1 & 0xFFFF0000u);
        }
    };
    // the wave's scores against the staged K tile: acc[b][r] = scale * (key 16 b + 4 l4 + r of the tile) . (query l15).  One chain per block, the same in both sweeps
    auto scores = [&](aps4_t (&acc)[NB]) {
#pragma unroll
        for (int b = 0; b < NB; b++) acc[b] = aps4_t{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ks = 0; ks < KSQ; ks++)
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const int row = 16 * b + l15;
                const aps8_t kf = *reinterpret_cast<const aps8_t *>(Kt + row * HD + (((4 * ks + l4) ^ (row & (C8 - 1))) << 3));
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], acc[b], 0, 0, 0);
            }
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc[b][r] = __fmul_rn(acc[b][r], scale);
    };
    // ---- sweep 1: the maximum of every query's row
    float mx = -INFINITY;
    Stage xk = k_load(0);
    for (int kt = 0; kt < nkt; kt++) {
        __syncthreads();
        k_write(xk);
        xk = k_load(kt + 1);
        __syncthreads();
        if (kt * APS_KT <= wlast) {
            aps4_t acc[NB];
            scores(acc);
            const int lim = qpos - kt * APS_KT - 4 * l4;              // key 16 b + r of the lane's part of the tile is seen when 16 b + r <= lim
#pragma unroll
            for (int b = 0; b < NB; b++)
#pragma unroll
                for (int r = 0; r < 4; r++) mx = fmaxf(mx, 16 * b + r <= lim ? acc[b][r] : -INFINITY);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16)); mx = fmaxf(mx, __shfl_xor(mx, 32));      // key 0 is seen by every query: finite
    // ---- sweep 2: exponentials, their sum, O^T += V^T e^T
    aps4_t oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; dt++) oacc[dt] = aps4_t{0.0f, 0.0f, 0.0f, 0.0f};
    double sum = 0.0;
    xk = k_load(0);
    Stage xv = v_load(0);
    for (int kt = 0; kt < nkt; kt++) {
        __syncthreads();
        k_write(xk);
        v_write(xv);
        xk = k_load(kt + 1);
        xv = v_load(kt + 1);
        __syncthreads();
        if (kt * APS_KT <= wlast) {
            aps4_t acc[NB];
            scores(acc);
            const int lim = qpos - kt * APS_KT - 4 * l4;
            aps8_t pf[NB / 2];
#pragma unroll
            for (int b = 0; b < NB; b++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const bool seen = 16 * b + r <= lim;
                    const float ev = exp_h(tb.exp, seen ? __fsub_rn(acc[b][r], mx) : 0.0f);
                    const float e = seen ? ev : 0.0f;
                    sum += (double)e;
                    pf[b >> 1][4 * (b & 1) + r] = (_Float16)e;
                }
#pragma unroll
            for (int dt = 0; dt < DT; dt++)
#pragma unroll
                for (int k2 = 0; k2 < NB / 2; k2++) {
                    const unsigned *vp = Vt + (16 * dt + l15) * APS_W + 16 * k2 + 2 * l4;      // dim 16 dt + l15: keys 32 k2 + 4 l4 .. + 3 and the same 16 keys on
                    union { uint2 u[2]; aps8_t v; } vb;
                    vb.u[0] = *reinterpret_cast<const uint2 *>(vp); vb.u[1] = *reinterpret_cast<const uint2 *>(vp + 8);
                    oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vb.v, pf[k2], oacc[dt], 0, 0, 0);
                }
        }
    }
    sum += __shfl_xor(sum, 16); sum += __shfl_xor(sum, 32);        // exact: fp16 values in a double, whatever the order
    const float inv = (float)(1.0 / sum);
    if (qrow < N) {
        float *op = out + (size_t)qrow * E + (size_t)h * HD + 4 * l4;
#pragma unroll
        for (int dt = 0; dt < DT; dt++)
            *reinterpret_cast<float4 *>(op + 16 * dt) = make_float4(__fmul_rn(oacc[dt][0], inv), __fmul_rn(oacc[dt][1], inv), __fmul_rn(oacc[dt][2], inv), __fmul_rn(oacc[dt][3], inv));
    }
}

AttnPrefillSKernel attn_prefill_s_kernel(int hd) {
    return hd == 128 ? &k_attn_prefill_s<128> : hd == 64 ? &k_attn_prefill_s<64> : hd == 32 ? &k_attn_prefill_s<32> : nullptr;
}

}  // namespace mg4
